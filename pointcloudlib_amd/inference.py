"""Frozen inference for the PointNet++ classifiers: ``frozen(net)`` evaluates a trained ``PointNet2_cls`` / ``PointNetMSG`` the way
``net.eval()`` under ``torch.no_grad()`` does (the reference's ``evaluate``, train_cls.py:92-124), on kernels made for it.

The eval constants are snapshot once on the device (per layer ``scale = gamma / sqrt(running_var + eps)``, ``shift = beta -
scale * running_mean``, folded conv bias; dense weights), so a forward launches no small torch ops and computes no BatchNorm
statistics.  Per ball-query set-abstraction level and scale: the per-point product ``Uf = feat W0[:, 3:]^T`` of the folded first
layer (stats-free library GEMM; narrow features such as SA1's normals fold inline instead), then ONE ``pcl_sa_level_infer_f32``
launch that runs the whole MLP + max of every group with its activations in LDS and writes its column slice of the level's output.
The GroupAll level runs the library's forward GEMMs stats-free with the snapshot constants, then its max; the head runs the
eval-mode head kernels on at most 64 rows per call.  A level whose shape has no fused kernel runs an eval-mode copy of its own
module.  ``net`` itself is never modified (parameters, running statistics, ``training`` flags)."""
import copy
import ctypes

import torch

from . import _lib
from .misc.head import MAX_ROWS, fc_head
from .misc.ops import _p, _stream, group_all, group_points
from .networks.cls.pointnet2 import PointNet2_cls

__all__ = ["frozen", "FrozenPointNet2"]


def frozen(net):
    """A frozen evaluator of ``net`` (``PointNet2_cls`` or ``PointNetMSG``): ``fnet(xyz, feature, sampling=None) -> [B, n_classes]``."""
    if not isinstance(net, PointNet2_cls):
        raise TypeError(f"frozen() takes PointNet2_cls or PointNetMSG (PointNet++ classification), got {type(net).__name__}")
    return FrozenPointNet2(net)


def _eval_consts(mlp, l):
    """(scale, shift) of layer ``l`` of a PointwiseMLP in evaluation mode, conv bias folded into the shift (fp32, on the device)."""
    W = mlp.weights[l]
    bias = None if mlp.biases is None else mlp.biases[l].detach()
    if mlp.bn:
        rm, rv = getattr(mlp, f"running_mean_{l}"), getattr(mlp, f"running_var_{l}")
        scale = mlp.gammas[l].detach() * torch.rsqrt(rv + mlp.eps)
        shift = mlp.betas[l].detach() - scale * (rm if bias is None else rm - bias)
    else:
        scale = torch.ones(W.shape[0], device=W.device)
        shift = torch.zeros(W.shape[0], device=W.device) if bias is None else bias.clone()
    return scale.float().contiguous(), shift.float().contiguous()


class _Fused:
    """Snapshot of one ball-query scale for pcl_sa_level_infer_f32."""

    def __init__(self, mlp, use_xyz, C):
        W0 = mlp.weights[0].detach().float().contiguous().clone()
        self.use_xyz, self.C, self.slope = use_xyz, C, float(mlp.slope)
        off = 3 if use_xyz else 0
        self.widths = [w.shape[0] for w in mlp.weights]
        self.W0 = W0
        self.ldw = W0.shape[1]
        self.Wx = W0[:, :3] if use_xyz else None                       # view: the kernel reads it with the row stride ldw
        self.inline = 0 < C <= 4
        self.Wf = None if C == 0 else (W0[:, off:] if self.inline else W0[:, off:].contiguous())
        self.Ws = [None] + [mlp.weights[l].detach().float().contiguous().clone() for l in range(1, len(self.widths))]
        consts = [_eval_consts(mlp, l) for l in range(len(self.widths))]
        self.scales, self.shifts = [c[0] for c in consts], [c[1] for c in consts]
        L = len(self.widths)
        self.c_widths = (ctypes.c_int32 * L)(*self.widths)
        self.c_W = (ctypes.c_void_p * L)(*[None if w is None else w.data_ptr() for w in self.Ws])
        self.c_scale = (ctypes.c_void_p * L)(*[t.data_ptr() for t in self.scales])
        self.c_shift = (ctypes.c_void_p * L)(*[t.data_ptr() for t in self.shifts])

    def run(self, xyz, new_xyz, feature, idx, cnt, out, col0):
        B, N, _ = xyz.shape
        m, ns = idx.shape[1], idx.shape[2]
        C1 = self.widths[0]
        st = _stream()
        feat2 = feature.reshape(B * N, self.C).contiguous() if self.C else None
        Uf = None
        if self.C and not self.inline:
            Uf = torch.empty((B * N, C1), dtype=torch.float32, device=xyz.device)
            _lib.call("pcl_linear_fwd_rows_f32", _p(feat2), _p(self.Wf), None, None, None, 0.0, B * N, self.C, C1, _p(Uf), None, None, None,
                      st, tag=f"pt{self.C}x{C1}")
        _lib.call("pcl_sa_level_infer_f32", _p(xyz), _p(new_xyz), _p(Uf), _p(self.Wx), _p(feat2) if self.inline else None,
                  _p(self.Wf) if self.inline else None, self.C if self.inline else 0, self.ldw, _p(idx), _p(cnt), B, N, m, ns,
                  len(self.widths), self.c_widths, self.c_W, self.c_scale, self.c_shift, self.slope, _p(out), out.shape[-1], col0, st)


class _GroupAllPlan:
    """Snapshot of the GroupAll level: dense weights and eval constants of every layer."""

    def __init__(self, mlp, use_xyz):
        self.use_xyz, self.slope, self.last_act = use_xyz, float(mlp.slope), mlp.last_act
        self.Ws = [w.detach().float().contiguous().clone() for w in mlp.weights]
        consts = [_eval_consts(mlp, l) for l in range(len(self.Ws))]
        self.scales, self.shifts = [c[0] for c in consts], [c[1] for c in consts]

    def run(self, xyz, feature):
        B, N, _ = xyz.shape
        dev = xyz.device
        st = _stream()
        cur = group_all(xyz, feature, self.use_xyz).reshape(B * N, -1)
        P = B * N
        sc = sh = None
        for W, scale, shift in zip(self.Ws, self.scales, self.shifts):
            cout, cin = W.shape
            Y = torch.empty((P, cout), dtype=torch.float32, device=dev)
            _lib.call("pcl_linear_fwd_rows_f32", _p(cur), _p(W), None, _p(sc), _p(sh), self.slope, P, cin, cout, _p(Y), None, None, None, st,
                      tag=f"fwd{cin}x{cout}")
            cur, sc, sh = Y, scale, shift
        C = cur.shape[1]
        out = torch.empty((B, C), dtype=torch.float32, device=dev)
        arg = torch.empty((B, C), dtype=torch.int32, device=dev)
        ymax = torch.empty((B, C), dtype=torch.float32, device=dev)
        _lib.call("pcl_bn_act_max_f32", _p(cur), _p(sc), _p(sh), self.slope if self.last_act else 1.0, B, N, C, _p(out), _p(arg), _p(ymax), st)
        return out.view(B, 1, C)


def _fusable(mlp, use_xyz, C, ns):
    if not (mlp.n_layers >= 2 and mlp.last_act and (use_xyz or C) and mlp.weights[0].shape[1] == (3 if use_xyz else 0) + C):
        return False
    widths = [w.shape[0] for w in mlp.weights] + [0] * (4 - mlp.n_layers)
    return mlp.n_layers <= 4 and bool(_lib.size_query("pcl_sa_level_infer_supported", int(ns), mlp.n_layers, *widths[:4]))


class FrozenPointNet2:
    """See the module docstring.  ``refresh()`` re-reads weights and running statistics from the network."""

    def __init__(self, net):
        self.net = net
        self._copies = {}          # eval-mode copies of the head and of levels without a fused kernel, kept across refresh()
        self.refresh()

    def _copy(self, key, module):
        c = self._copies.get(key)
        if c is None:
            c = self._copies[key] = copy.deepcopy(module).eval()
        else:
            c.load_state_dict(module.state_dict())        # same objects: the head kernels' plan cache keys on them
        return c

    @torch.no_grad()
    def refresh(self):
        net = self.net
        C = 3                      # the classifiers' input feature: the normals (PointNet2_cls.forward(xyz, feature))
        self.levels = []
        for i, module in enumerate(net.pointnet_modules):
            plans = []
            for j, (grouper, mlp) in enumerate(zip(module.groupers, module.mlps)):
                use_xyz = bool(grouper.use_xyz)
                if module.n_points is None:
                    plans.append(("all", _GroupAllPlan(mlp, use_xyz)))
                elif _fusable(mlp, use_xyz, C, grouper.n_samples):
                    plans.append(("fused", _Fused(mlp, use_xyz, C)))
                else:
                    plans.append(("module", self._copy((i, j), mlp)))
            self.levels.append(plans)
            C = sum(mlp.spec[-1] for mlp in module.mlps)
        self.head = self._copy("head", net.fc_layer)
        return self

    def __call__(self, xyz, feature, sampling=None):
        return self.run(xyz, feature, sampling)[1]

    @torch.no_grad()
    def run(self, xyz, feature, sampling=None):
        """-> ([feature of every set-abstraction level], logits [B, n_classes])."""
        net = self.net
        net.adopt_sampling(sampling)
        feats = []
        for i, (module, plans) in enumerate(zip(net.pointnet_modules, self.levels)):
            s = sampling["levels"][i] if sampling is not None else module.sample(xyz)
            xyz, feature = self._level(module, plans, xyz, feature, s)
            feats.append(feature)
        feature = feature.squeeze(dim=1)
        logits = [fc_head(self.head, feature[r:r + MAX_ROWS]) for r in range(0, feature.shape[0], MAX_ROWS)]
        return feats, logits[0] if len(logits) == 1 else torch.cat(logits)

    def _level(self, module, plans, xyz, feature, s):
        new_xyz, idxs = s
        xyz = xyz.contiguous()
        if new_xyz is None:                                 # GroupAll
            (kind, plan), = plans
            return None, plan.run(xyz, feature)
        B = xyz.shape[0]
        m = new_xyz.shape[1]
        new_xyz = new_xyz.contiguous()
        feature = None if feature is None else feature.contiguous()
        width = sum(mlp.spec[-1] for mlp in module.mlps)
        out = torch.empty((B, m, width), dtype=torch.float32, device=xyz.device)
        col = 0
        for (kind, plan), grouper, mlp, ic in zip(plans, module.groupers, module.mlps, idxs):
            cl = mlp.spec[-1]
            if kind == "fused":
                plan.run(xyz, new_xyz, feature, ic[0], ic[1], out, col)
            else:
                if module.compact_duplicates and plan.resolved_backend(xyz) == "hip":
                    y = plan.forward_grouped(xyz, new_xyz, feature, ic[0], ic[1], ic[2], grouper.use_xyz)
                else:
                    grouped = group_points(xyz, new_xyz, feature, ic[0], grouper.use_xyz)
                    y = plan(grouped, group_max=grouped.shape[2])
                out[:, :, col:col + cl] = y
            col += cl
        return new_xyz, out
