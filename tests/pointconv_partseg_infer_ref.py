"""Shapes and the fp64 evaluation-mode restatement of PointConv part segmentation (networks/seg/pointconv_partseg.py) for the tests of
FrozenPointConvPartseg, on top of tests/pointconv_infer_ref.py.  Index lists, centres, densities and the 3-NN interpolation's
``idx3, w3`` are arguments (a handle of ``net.precompute_sampling``), so sampling is not part of what is compared.  Not a test file."""
import torch

import pointconv_infer_ref as R

EXACT_SEED = 0
# (ns, widths, point features D, B, N, m) per new kernel shape: 15 groups (the last tile partly filled: 1 of 2 groups at ns = 32, 3 of
# 4 at ns = 16), tiles straddle clouds, N % 4 != 0; Uf is formed outside the kernel, so a small D serves
SHAPES = {"sa0": (32, [32, 32, 64], 0, 3, 41, 5), "sa2": (32, [128, 128, 256], 8, 3, 41, 5),
          "in1": (16, [256, 256], 8, 3, 41, 5), "in2": (16, [128, 128], 8, 3, 41, 5), "in3": (16, [128, 128, 128], 8, 3, 41, 5)}
# enough groups that a workgroup owns several tiles on an MI355X while the B = 1 launch of one cloud owns fewer (the tests assert
# it); G = 8195 is odd: the last tile holds one group of two (ns = 32), three of four (ns = 16)
MANY = {"sa0": (32, [32, 32, 64], 0, 5, 41, 1639), "in3": (16, [128, 128, 128], 8, 5, 41, 1639)}
LEVELS = ("sa0", "sa1", "sa2", "sa3", "in0", "in1", "in2", "in3")


def stacks_of(level):
    return R.stack_of(level.mlp), R.stack_of(level.weightnet.mlp), R.stack_of(level.densitynet.mlp)


def network(net, xyz, levels):
    """fp64 evaluation of PointConvDensity_partseg on ``levels`` (what ``net.precompute_sampling(xyz)["levels"]`` holds); xyz [B,N,3]
    -> ([the eight level outputs, channel-last], logits [B,N,part_num]).  Wired as networks/seg/pointconv_partseg.py: an
    interpolation level's output rows are in its FPS visiting order and are read by the next level in that order."""
    B = xyz.shape[0]
    bidx = torch.arange(B, device=xyz.device).view(B, 1, 1)
    pts, points, feats = [xyz], None, []
    for name, (new_xyz, ((idx, density),)) in zip(LEVELS[:4], levels[:4]):
        sa = getattr(net, name)
        out = R.level(*stacks_of(sa), pts[-1], new_xyz, points, idx, density, sa.mlp.slope)
        points = R.run_stack(R.stack_of(sa.linear), out, sa.linear.slope, torch.float64)
        feats.append(points)
        pts.append(new_xyz)
    for k, (name, s) in enumerate(zip(LEVELS[4:], levels[4:])):
        lv = getattr(net, name)
        interpolated = (s["w3"].double().unsqueeze(-1) * points[bidx, s["idx3"].long()]).sum(dim=2)
        out = R.level(*stacks_of(lv), pts[3 - k], s["new_xyz"], interpolated, s["idx"], s["density"], lv.mlp.slope)
        points = R.run_stack(R.stack_of(lv.linear), out, lv.linear.slope, torch.float64)
        feats.append(points)
    x = R.run_stack(R.stack_of(net.fc1), points, net.fc1.slope, torch.float64)
    return feats, x @ net.fc3.weight.double().t() + net.fc3.bias.double()
