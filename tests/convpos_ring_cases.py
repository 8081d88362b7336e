"""Cases and the expected route of f5_convpos_ring_kernel (csrc/convpos.hip), shared by tests/test_convpos_ring_gpu.py (launches them)
and tests/test_convpos_ring_host.py (checks the cover and the route on the CPU).  The data, the buffers and the fp64 bound are those
of tests/convaudio_matrix.py: a case here is one of its conv-pos cases with a selector of 8.

The cover: ten data sets, each run in mode 0 with the lo output, mode 0 without it and mode 1, so that every value below meets every
mode.  They are the smallest shapes at which a ring or a swizzle can go wrong:
    taps  1, 3, 5      fewer slabs than the ring requests ahead: nothing but the prologue's requests, the wave drains at once
          29, 31       the ring wraps (8 slots) and the last slabs arrive while nothing more is requested
    N     1, 16        a halo shorter than the tile, zero rows on both sides at once; 127 / 128 / 129: the tile's edge; 129 and 257: a last
                       tile whose waves 1-3 have no row at all
    B     1, 3         per-element zero padding; the 1-D decode of (token tile, element)
    C     64           one group: a 3-D grid, with several token tiles (257, 129) that must not be decoded as the 1-D numbering
          512, 1024    8 and 16 groups, under the 1-D group-per-XCD numbering and the plain one
    var   neighbours   an element between neighbours 1e3 times larger: a halo row read from the wrong element shows
          mish         pre-activations at the clamp of f5_mish
"""
import convaudio_matrix as CM

TAPS = (1, 3, 5, 29, 31)
NS = (1, 16, 127, 128, 129, 257)
BS = (1, 3)
CS = (64, 512, 1024)
VARS = ("normal", "neighbours", "mish")
OUTS = CM.CP_OUTS                                        # (mode, lo): (0, 1), (0, 0), (1, 0)
RING, TWIN = 8, 1                                        # selectors: the ring kernel, f5_convpos_kernel<false,1>

# (C, N, B, taps, var, xcd)
DATA = (
    (64, 1, 1, 1, "normal", 1),
    (512, 16, 3, 3, "neighbours", 1),
    (1024, 127, 1, 5, "normal", 0),
    (1024, 128, 3, 29, "mish", 1),
    (512, 129, 1, 31, "normal", 0),
    (1024, 257, 3, 31, "neighbours", 1),
    (64, 257, 3, 29, "mish", 0),
    (512, 257, 1, 5, "normal", 1),
    (1024, 16, 1, 3, "mish", 1),
    (64, 129, 1, 31, "normal", 1),
)
RACE = (1024, 257, 3, 31, "normal", 1)                   # launched twenty times under the ring selector
RACE_LAUNCHES = 20


def case(data, tps, mode, lo):
    C, N, B, taps, var, xcd = data
    return CM._cp(C, N, B, taps, 1, tps, xcd, mode, lo, var)


def twins():
    """[(ring case, twin case)]: the same data and outputs under selector 8 and selector 1"""
    return [(case(d, RING, mode, lo), case(d, TWIN, mode, lo)) for d in DATA for (mode, lo) in OUTS]


def kernel_name(C, N, B, nseg=1, tps=0, xcd=1):
    """what f5_debug_last_convpos_kernel must report (csrc/convpos.hip f5_convpos_route).  Automatic route to the ring kernel: one
    segment, groups dealt to XCDs, at least 512 tokens, a grid of one round (at most 256 workgroups of 128 tokens x one group)."""
    groups = C // 64
    dealt = groups % 8 == 0 and bool(xcd)
    nwg = -(-N // 128) * groups * B
    if nseg == 3:
        name = f"f5_convpos_kernel<true,{min(tps or 1, 2)}>"
    elif tps == RING or (tps == 0 and dealt and N >= 512 and nwg <= 256):
        name = "f5_convpos_ring_kernel"
    else:
        name = f"f5_convpos_kernel<false,{tps or 1}>"
    return name + ("+xcd" if dealt else "")


# (C, N, B, nseg, tps) -> the name the issue fixes for it
ROUTES = (
    ((1024, 937, 2, 1, 0), "f5_convpos_ring_kernel+xcd"),          # the benchmark's batch 1: 8 x 16 x 2 = 256 workgroups
    ((1024, 257, 3, 1, 0), "f5_convpos_kernel<false,1>+xcd"),      # short sequence
    ((1024, 937, 2, 3, 0), "f5_convpos_kernel<true,1>+xcd"),       # three segments
    ((64, 937, 1, 1, 0), "f5_convpos_kernel<false,1>"),            # one group: no dealing to XCDs
    ((1024, 937, 2, 3, 8), "f5_convpos_kernel<true,2>+xcd"),       # the ring selector with three segments
)
