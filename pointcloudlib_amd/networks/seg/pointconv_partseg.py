"""PointConv part segmentation -- counterpart of /root/reference/networks/seg/pointconv_partseg.py:9-63.

Four ``PointConvDensitySetAbstraction`` levels (1024/256/64/36 points, 32 neighbours), four
``PointConvDensitySetInterpolation`` levels back up (16 neighbours), head Conv1d 128->128 + BN + ReLU + Dropout 0.4
+ Conv1d 128->part_num.  ``xyz`` is ``[B,N,3]`` (permuted at :42) and the output ``[B,N,part_num]`` (:61);
``cls_label`` is accepted and unused, as upstream."""
import torch
from torch import nn

from ...misc.layers import PointwiseMLP
from ...misc.pointconv_utils import PointConvDensitySetAbstraction, PointConvDensitySetInterpolation


class PointConvDensity_partseg(nn.Module):
    def __init__(self, part_num=50):
        super().__init__()
        self.part_num = part_num
        SA, IN = PointConvDensitySetAbstraction, PointConvDensitySetInterpolation
        self.sa0 = SA(npoint=1024, nsample=32, in_channel=3, mlp=[32, 32, 64], bandwidth=0.1, group_all=False)
        self.sa1 = SA(npoint=256, nsample=32, in_channel=64 + 3, mlp=[64, 64, 128], bandwidth=0.2, group_all=False)
        self.sa2 = SA(npoint=64, nsample=32, in_channel=128 + 3, mlp=[128, 128, 256], bandwidth=0.4, group_all=False)
        self.sa3 = SA(npoint=36, nsample=32, in_channel=256 + 3, mlp=[256, 256, 512], bandwidth=0.8, group_all=False)
        self.in0 = IN(nsample=16, in_channel=512 + 3, mlp=[512, 512], bandwidth=0.8)
        self.in1 = IN(nsample=16, in_channel=512 + 3, mlp=[256, 256], bandwidth=0.4)
        self.in2 = IN(nsample=16, in_channel=256 + 3, mlp=[128, 128], bandwidth=0.2)
        self.in3 = IN(nsample=16, in_channel=128 + 3, mlp=[128, 128, 128], bandwidth=0.1)
        self.fc1 = PointwiseMLP([128, 128], bias=True)               # fc1 + bn1 + relu  :36-37,:58
        self.drop1 = nn.Dropout(0.4)
        self.fc3 = nn.Linear(128, part_num)

    LEVELS = ("sa0", "sa1", "sa2", "sa3", "in0", "in1", "in2", "in3")            # in call order

    @torch.no_grad()
    def precompute_sampling(self, xyz, start_idx=None):
        """Everything of a batch that depends on its coordinates only, per level in call order (``LEVELS``): ``sa.sample`` of the four
        set-abstraction levels, ``PointConvDensitySetInterpolation.sample`` of the four interpolation levels.  xyz [B,N,3] (the
        layout ``forward`` takes); ``start_idx``: eight [B] int32 FPS starts in call order (default: drawn at random, as ``forward``
        does).  Runs on the current stream; returns a handle for ``forward(xyz, sampling=handle)``."""
        starts = [None] * 8 if start_idx is None else list(start_idx)
        if len(starts) != 8:
            raise ValueError(f"precompute_sampling: start_idx must hold eight [B] tensors ({', '.join(self.LEVELS)}), got {len(starts)}")
        pts = [xyz.contiguous()]                                      # l0 .. l4 coordinates, channel-last
        levels = []
        for name, s in zip(self.LEVELS[:4], starts[:4]):
            lv = getattr(self, name).sample(pts[-1], s)
            levels.append(lv)
            pts.append(lv[0])
        for k, (name, s) in enumerate(zip(self.LEVELS[4:], starts[4:])):
            levels.append(getattr(self, name).sample(pts[3 - k], pts[4 - k], s))
        return {"levels": levels, "event": None}

    def forward(self, xyz, cls_label=None, sampling=None):
        """``sampling``: a handle of ``precompute_sampling(xyz)``."""
        lv = [None] * 8 if sampling is None else sampling["levels"]
        xyz = xyz.permute(0, 2, 1).contiguous()                       # [B,3,N]  :42
        l1_xyz, l1_points = self.sa0(xyz, None, sampling=lv[0])
        l2_xyz, l2_points = self.sa1(l1_xyz, l1_points, sampling=lv[1])
        l3_xyz, l3_points = self.sa2(l2_xyz, l2_points, sampling=lv[2])
        l4_xyz, l4_points = self.sa3(l3_xyz, l3_points, sampling=lv[3])
        l3_points = self.in0(l3_xyz, l4_xyz, l3_points, l4_points, sampling=lv[4])    # :51-54
        l2_points = self.in1(l2_xyz, l3_xyz, l2_points, l3_points, sampling=lv[5])
        l1_points = self.in2(l1_xyz, l2_xyz, l1_points, l2_points, sampling=lv[6])
        l0_points = self.in3(xyz, l1_xyz, xyz, l1_points, sampling=lv[7])
        x = self.drop1(self.fc1(l0_points.permute(0, 2, 1).contiguous()))   # [B,N,128]
        return self.fc3(x)                                            # [B,N,part_num]  :59-61

    def execute(self, *a, **k):
        return self(*a, **k)
