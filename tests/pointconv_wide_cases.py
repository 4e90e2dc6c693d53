"""Cases of the wide PointConv level kernel (pcl_pointconv_wide_level_infer_f32; ``FrozenPointConvPartseg(net, wide_levels=True)``)
for tests/test_inference_pointconv_wide_{cpu,gpu}.py.  Not a test file."""
WIDE = "pcl_pointconv_wide_level_infer_f32"
SUPPORTED_QUERY = "pcl_pointconv_wide_level_infer_supported"
GROUP_TILE = "pcl_pointconv_wide_level_infer_group_tile"
# (ns, widths, point features D, B, N, m): 15 groups -- the last tile partly filled (1 of 2 groups at ns = 32, 3 of 4 at ns = 16),
# tiles straddle clouds; D = 8 keeps Uf in play (the kernel does not see D)
SHAPES = {"sa3": (32, [256, 256, 512], 8, 3, 41, 5), "in0": (16, [512, 512], 8, 3, 41, 5)}
# (ns, L, C1, C2, C3) of the queries: C2 = widths[1], C3 = widths[L-1]
SUPPORTED = {(32, 3, 256, 256, 512), (16, 2, 512, 512, 512)}
ALL_FUSED = ["fused"] * 8
STOCK = ["fused", "fused", "fused", "module", "module", "fused", "fused", "fused"]
MANY_B, MANY_N, MANY_M_END = 5, 41, 1639
# the seed of the many-tiles cases' exact data.  The generator's draws depend on the sizes, and at sa3's m on 256 compute units (103)
# EXACT_SEED = 0 leaves the contraction's audit at 2^24.4 -- over the 2^24 below which every partial sum is an fp32 number in any
# order; seed 1 gives 2^19.7 (sa3, m = 103) and 2^21.5 (in0, m = 205) at nonzero shares 0.46 and 0.64 (the CPU file asserts it)
MANY_SEED = 1


def many_m(group_tile, ns, B=MANY_B):
    """The smallest m below MANY_M_END at which a launch over B * m groups gives a workgroup at least two tiles (``group_tile``: the
    library's query) and leaves the last tile partly filled; None if there is none."""
    gpt = 64 // ns
    for m in range(1, MANY_M_END):
        if group_tile(ns, B * m) >= 2 * gpt and (B * m) % gpt != 0:
            return m
    return None


def case_args(c):
    return c["xyz"], c["new_xyz"], c["points"], c["idx"], c["density"]
