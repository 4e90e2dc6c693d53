"""Frozen inference: evaluators that run a trained network the way ``net.eval()`` under ``torch.no_grad()`` does (the reference's
``evaluate``, train_cls.py:92-124), on kernels made for it.  Each class states its own plan; this is the index.

- ``FrozenPointNet2``: ``PointNet2_cls`` / ``PointNetMSG``, through ``frozen(net)``; csrc/infer.hip; DESIGN.md sections 12, 14
  (``lengths=``) and 17 (``precision="bf16"``).
- ``FrozenPointNet2Partseg``: ``PointNet2_partseg`` / its ``PointNetMSG``, through ``frozen(net)``; csrc/infer.hip and
  csrc/infer_fp.hip; DESIGN.md sections 13, 14 and 17.
- ``FrozenPointNet``: ``networks.cls.pointnet.PointNet``; csrc/infer_pointnet.hip; DESIGN.md sections 19 and 21 (bf16).
- ``FrozenPointNetPartseg``: ``networks.seg.pointnet_partseg.PointNet_partseg``; csrc/infer_pointnet_seg.hip; DESIGN.md sections 20
  and 23 (bf16).
- ``FrozenPointConv``: ``networks.cls.pointconv.PointConvDensityClsSsg``; csrc/infer_pointconv.hip; DESIGN.md sections 24 and 25
  (bf16).
- ``FrozenPointConvPartseg``: ``networks.seg.pointconv_partseg.PointConvDensity_partseg``; csrc/infer_pointconv.hip and
  csrc/infer_pointconv_seg_bf16.hip, csrc/infer_pointconv_wide.hip; DESIGN.md sections 26, 27 (bf16) and 28 (``wide_levels``).
- ``FrozenPointCNN``: ``networks.cls.pointcnn.PointCNNcls``; csrc/infer_xconv.hip; DESIGN.md section 29 (fp32 only).
- ``FrozenPointCNNPartseg``: ``networks.seg.pointcnn_partseg.PointCNN_partseg``; csrc/infer_xconv.hip and csrc/infer_xconv_seg.hip;
  DESIGN.md section 30 (fp32 only).

All but the two PointNet++ evaluators are constructed directly: ``frozen()`` keeps its PointNet++ dispatch."""
import copy
import ctypes

import torch

from . import _lib
from .misc.head import MAX_ROWS, fc_head
from .misc.layers import PointwiseMLP
from .misc.ops import (_lengths, _p, _stream, group_all, group_points, knn_indices, mlp_segment_max, pack_rows, packed_layout,
                       three_interpolate, three_nn, unpack_rows)
from .misc.pointcnn import Dense_Conv1d, RandPointCNN, RandPointCNN_Decoder
from .misc.pointconv_utils import (DensityNet, PointConvDensitySetAbstraction, PointConvDensitySetInterpolation, WeightNet, _linear_flush,
                                   _pointconv_linear, compute_density, sample_level)
from .networks.cls.pointcnn import PointCNNcls
from .networks.cls.pointconv import PointConvDensityClsSsg
from .networks.cls.pointnet import PointNet
from .networks.cls.pointnet2 import PointNet2_cls, SamplingPrefetch
from .networks.seg.pointcnn_partseg import PointCNN_partseg
from .networks.seg.pointconv_partseg import PointConvDensity_partseg
from .networks.seg.pointnet2_partseg import PointNet2_partseg
from .networks.seg.pointnet_partseg import PointNet_partseg

__all__ = ["frozen", "FrozenPointCNN", "FrozenPointCNNPartseg", "FrozenPointConv", "FrozenPointConvPartseg", "FrozenPointNet", "FrozenPointNet2", "FrozenPointNet2Partseg", "FrozenPointNetPartseg"]


PRECISIONS = ("fp32", "bf16")


def frozen(net, precision="fp32"):
    """A frozen evaluator of ``net``: ``PointNet2_cls`` or ``PointNetMSG`` (classification) -> ``fnet(xyz, feature, sampling=None,
    lengths=None) -> [B, n_classes]``; ``PointNet2_partseg`` or its ``PointNetMSG`` (part segmentation) -> ``fnet(xyz, feature,
    cls_label, sampling=None, lengths=None) -> [B, part_num, N]``.  ``lengths`` [B]: per-cloud point counts of a ragged batch
    (capacity N; rows from lengths[b] on are pad rows, any contents): every cloud's result is that of the cloud alone; the
    part-seg logits and ``fp1`` feature of pad points are exact zeros.  ``precision``: "fp32", or "bf16" for bf16 matrix operands
    in the fused set-abstraction launches (``_FrozenEncoder``); ``fnet.precision`` tells which."""
    if precision not in PRECISIONS:
        raise ValueError(f"frozen(): precision must be one of {PRECISIONS}, got {precision!r}")
    if isinstance(net, PointNet2_cls):
        return FrozenPointNet2(net, precision)
    if isinstance(net, PointNet2_partseg):
        return FrozenPointNet2Partseg(net, precision)
    raise TypeError(f"frozen() takes PointNet2_cls or PointNetMSG (PointNet++ classification) or PointNet2_partseg / its PointNetMSG "
                    f"(PointNet++ part segmentation), got {type(net).__name__}; PointNet has FrozenPointNet(net)")


def _eval_consts(mlp, l, fold_bias=True):
    """(scale, shift) of layer ``l`` of a PointwiseMLP in evaluation mode, conv bias folded into the shift (fp32, on the device).
    ``fold_bias=False``: the constants behind a GEMM that adds the bias itself."""
    W = mlp.weights[l]
    bias = None if mlp.biases is None or not fold_bias else mlp.biases[l].detach()
    if mlp.bn:
        rm, rv = getattr(mlp, f"running_mean_{l}"), getattr(mlp, f"running_var_{l}")
        scale = mlp.gammas[l].detach() * torch.rsqrt(rv + mlp.eps)
        shift = mlp.betas[l].detach() - scale * (rm if bias is None else rm - bias)
    else:
        scale = torch.ones(W.shape[0], device=W.device)
        shift = torch.zeros(W.shape[0], device=W.device) if bias is None else bias.clone()
    return scale.float().contiguous(), shift.float().contiguous()


def _pad32(t, fill):
    """``t`` ([C, ...] or [C]) with its first dimension padded to a multiple of 32 with ``fill``."""
    c = t.shape[0]
    cp = -(-c // 32) * 32
    if cp == c:
        return t.contiguous()
    out = torch.full((cp,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
    out[:c] = t
    return out


def _entry(name, precision):
    """The entry point ``name`` (``..._f32``) for ``precision``: the bf16-operand form of a launch is named ``..._bf16_f32``."""
    return name[:-len("f32")] + "bf16_f32" if precision == "bf16" else name


def _rows_gemm(X, W, bias=None, in_scale=None, in_shift=None, slope=0.0, tag="fwd"):
    """``act(in_scale * X + in_shift) W^T + bias`` -> [P, Cout]: the stats-free library GEMM (``pcl_linear_fwd_rows_f32``) on X [P, Cin]
    and W [Cout, Cin]; without ``in_scale`` X is taken as it is.  ``tag``: the profile key's prefix -- ``"pt"`` for the per-point
    product of a folded first layer, ``"fwd"`` for a layer of a chain."""
    P = X.shape[0]
    Cout, Cin = W.shape
    Y = torch.empty((P, Cout), dtype=torch.float32, device=X.device)
    _lib.call("pcl_linear_fwd_rows_f32", _p(X), _p(W), _p(bias), _p(in_scale), _p(in_shift), slope, P, Cin, Cout, _p(Y), None, None, None,
              _stream(), tag=f"{tag}{Cin}x{Cout}")
    return Y


_OWN = object()                   # _SegStack(first=_OWN): the first weight is the first layer's own


class _SegStack:
    """Snapshot of consecutive layers ``[(mlp, l)]`` for a frozen-inference launcher: dense fp32 weights ``Ws``, eval constants
    ``scales`` / ``shifts``, the layer ``widths``, and the ctypes arrays ``c_widths / c_W / c_scale / c_shift`` over them;
    ``operands`` is the list ``c_W`` points at.

    ``first``: what stands for the first weight -- by default a clone of the layer's own; ``None`` when the first layer is
    folded and the kernel takes it apart from the arrays (the clone is then ``W0``, for the caller to slice); or a tensor that
    replaces it.  ``bf16``: also ``Ws_bf16``, the weights of layers 2 and up rounded once to bf16 (``[None, ...]``), and ``c_W``
    points at those.  ``pad_last``: the last layer's weight, scale and shift padded to a multiple of 32 rows (zero weights);
    ``widths`` keeps the layer's own.  ``bf16_first`` (with ``bf16``): ALL layers as bf16 -- ``_OWN`` rounds the first layer's own
    weight like the others, a bf16 tensor stands for it (a folded weight its caller rounded straight from fp64); by default the
    first entry stays ``None``."""

    def __init__(self, layers, first=_OWN, bf16=False, pad_last=False, bf16_first=None):
        self.L = L = len(layers)
        self.widths = [mlp.weights[l].shape[0] for mlp, l in layers]
        self.Ws, self.scales, self.shifts = [], [], []
        for i, (mlp, l) in enumerate(layers):
            sc, sh = _eval_consts(mlp, l)
            W = mlp.weights[l].detach().float()
            if pad_last and i == L - 1:
                W, sc, sh = _pad32(W, 0.0), _pad32(sc, 1.0), _pad32(sh, 0.0)
            self.Ws.append(W.contiguous().clone() if i or first is _OWN else first)
            self.scales.append(sc)
            self.shifts.append(sh)
        if first is None:
            mlp, l = layers[0]
            self.W0 = mlp.weights[l].detach().float().contiguous().clone()
        self.operands = self.Ws
        if bf16:                                                       # the bf16 operands of layers 2 and up, rounded once here
            self.operands = self.Ws_bf16 = [None] + [w.to(torch.bfloat16).contiguous() for w in self.Ws[1:]]
            if bf16_first is not None:
                self.operands[0] = self.Ws[0].to(torch.bfloat16).contiguous() if bf16_first is _OWN else bf16_first
        self.c_widths = (ctypes.c_int32 * L)(*self.widths)
        self.c_W = (ctypes.c_void_p * L)(*[None if w is None else w.data_ptr() for w in self.operands])
        self.c_scale = (ctypes.c_void_p * L)(*[t.data_ptr() for t in self.scales])
        self.c_shift = (ctypes.c_void_p * L)(*[t.data_ptr() for t in self.shifts])


class _Fused(_SegStack):
    """Snapshot of one ball-query scale for pcl_sa_level_infer_f32 (or, ``precision="bf16"``, pcl_sa_level_infer_bf16_f32)."""

    def __init__(self, mlp, use_xyz, C, precision="fp32"):
        super().__init__([(mlp, l) for l in range(len(mlp.weights))], first=None, bf16=precision == "bf16")
        self.precision = precision
        self.use_xyz, self.C, self.slope = use_xyz, C, float(mlp.slope)
        W0, off = self.W0, 3 if use_xyz else 0
        self.ldw = W0.shape[1]
        self.Wx = W0[:, :3] if use_xyz else None                       # view: the kernel reads it with the row stride ldw
        self.inline = 0 < C <= 4
        self.Wf = None if C == 0 else (W0[:, off:] if self.inline else W0[:, off:].contiguous())
        self.entry = _entry("pcl_sa_level_infer_f32", precision)

    def run(self, xyz, new_xyz, feature, idx, cnt, out, col0):
        B, N, _ = xyz.shape
        m, ns = idx.shape[1], idx.shape[2]
        feat2 = feature.reshape(B * N, self.C).contiguous() if self.C else None
        Uf = _rows_gemm(feat2, self.Wf, tag="pt") if self.C and not self.inline else None
        _lib.call(self.entry, _p(xyz), _p(new_xyz), _p(Uf), _p(self.Wx), _p(feat2) if self.inline else None,
                  _p(self.Wf) if self.inline else None, self.C if self.inline else 0, self.ldw, _p(idx), _p(cnt), B, N, m, ns,
                  len(self.widths), self.c_widths, self.c_W, self.c_scale, self.c_shift, self.slope, _p(out), out.shape[-1], col0, _stream())


class _RowsStack:
    """Snapshot of a PointwiseMLP for the stats-free library GEMMs: dense weights and eval constants (conv bias folded into the
    shift).  ``run(x [P, C0])`` chains ``_rows_gemm`` with the BatchNorm + activation of each layer folded into the next GEMM's
    operand load -> (pre-BatchNorm output of the last layer, its scale, its shift); ``run_act`` applies them too."""

    def __init__(self, mlp):
        self.slope = float(mlp.slope)
        self.out_slope = self.slope if mlp.last_act else 1.0
        self.Ws = [w.detach().float().contiguous().clone() for w in mlp.weights]
        consts = [_eval_consts(mlp, l) for l in range(len(self.Ws))]
        self.scales, self.shifts = [c[0] for c in consts], [c[1] for c in consts]

    def run(self, cur):
        sc = sh = None
        for W, scale, shift in zip(self.Ws, self.scales, self.shifts):
            cur, sc, sh = _rows_gemm(cur, W, None, sc, sh, self.slope), scale, shift
        return cur, sc, sh

    def run_act(self, x):
        Y, sc, sh = self.run(x)
        out = torch.empty_like(Y)
        _lib.call("pcl_bn_act_f32", _p(Y), _p(sc), _p(sh), self.out_slope, Y.shape[0], Y.shape[1], _p(out), _stream())
        return out


class _GroupAllPlan:
    """Snapshot of the GroupAll level: the MLP as a chain of stats-free GEMMs (``_RowsStack``), then the BatchNorm + activation
    of its last layer and the max over the cloud's points in one launch (``pcl_bn_act_max_f32``)."""

    def __init__(self, mlp, use_xyz):
        self.use_xyz, self.stack = use_xyz, _RowsStack(mlp)

    def run(self, xyz, feature):
        B, N, _ = xyz.shape
        Y, sc, sh = self.stack.run(group_all(xyz, feature, self.use_xyz).reshape(B * N, -1))
        C = Y.shape[1]
        out = torch.empty((B, C), dtype=torch.float32, device=xyz.device)
        arg = torch.empty((B, C), dtype=torch.int32, device=xyz.device)
        ymax = torch.empty((B, C), dtype=torch.float32, device=xyz.device)
        _lib.call("pcl_bn_act_max_f32", _p(Y), _p(sc), _p(sh), self.stack.out_slope, B, N, C, _p(out), _p(arg), _p(ymax), _stream())
        return out.view(B, 1, C)


def _fusable(mlp, use_xyz, C, ns):
    if not (mlp.n_layers >= 2 and mlp.last_act and (use_xyz or C) and mlp.weights[0].shape[1] == (3 if use_xyz else 0) + C):
        return False
    widths = [w.shape[0] for w in mlp.weights] + [0] * (4 - mlp.n_layers)
    return mlp.n_layers <= 4 and bool(_lib.size_query("pcl_sa_level_infer_supported", int(ns), mlp.n_layers, *widths[:4]))


class _Frozen:
    """What the evaluators share.  ``NET``: the network class an evaluator takes.  The eval constants are snapshot once on the device
    by ``refresh()`` (per layer ``scale = gamma / sqrt(running_var + eps)``, ``shift = beta - scale * running_mean``, folded conv
    bias; dense weights), so a forward launches no small torch ops and computes no BatchNorm statistics; ``net`` itself is never
    modified (parameters, running statistics, ``training`` flags)."""

    NET = None

    def __init__(self, net, precision="fp32"):
        name = type(self).__name__
        if not isinstance(net, self.NET):
            raise TypeError(f"{name} takes {self.NET.__module__.split('.', 1)[1]}.{self.NET.__name__}, got {type(net).__name__}")
        if precision not in PRECISIONS:
            raise ValueError(f"{name}: precision must be one of {PRECISIONS}, got {precision!r}")
        self.net = net
        self.precision = precision
        self._copies = {}          # eval-mode copies of the heads and of modules without a fused kernel, kept across refresh()
        self.refresh()

    def _copy(self, key, module):
        c = self._copies.get(key)
        if c is None:
            c = self._copies[key] = copy.deepcopy(module).eval()
        else:
            c.load_state_dict(module.state_dict())        # same objects: the head kernels' plan cache keys on them
        return c

    def _require_f32_gpu(self, x, what="tensor"):
        if not x.is_cuda or x.dtype != torch.float32:
            raise TypeError(f"{type(self).__name__}: expected a float32 {what} on the GPU, got {x.dtype} on {x.device}")

    def _fc_head(self, feature):
        """``self.head`` (the eval-mode head kernels) on the rows of ``feature``, at most ``MAX_ROWS`` of them per call."""
        logits = [fc_head(self.head, feature[r:r + MAX_ROWS]) for r in range(0, feature.shape[0], MAX_ROWS)]
        return logits[0] if len(logits) == 1 else torch.cat(logits)


class _FrozenEncoder(_Frozen):
    """The set-abstraction levels of a PointNet++ network (``net.pointnet_modules``, input feature 3 wide): a plan per level and
    scale, and the eval-mode copies of modules without a fused kernel.  Shared by the classification and part-seg evaluators.

    Per ball-query level and scale: the per-point product ``Uf = feat W0[:, 3:]^T`` of the folded first layer (stats-free library
    GEMM; narrow features such as SA1's normals fold inline instead), then ONE ``pcl_sa_level_infer_f32`` launch that runs the whole
    MLP + max of every group with its activations in LDS and writes its column slice of the level's output.  The GroupAll level runs
    the library's forward GEMMs stats-free with the snapshot constants, then its max.  A level whose shape has no fused kernel runs
    an eval-mode copy of its own module.

    ``precision="bf16"`` runs every fused set-abstraction launch as ``pcl_sa_level_infer_bf16_f32``: layers 2 and up take bf16
    operands (activations rounded to nearest even, weights snapshot as bf16 once) and accumulate in fp32; the first layer, ``Uf``,
    the epilogues, the max and every output stay fp32, and so do the GroupAll level, the FP levels and the heads."""

    def _refresh_encoder(self):
        net = self.net
        C = 3                      # the input feature: the normals (forward(xyz, feature, ...))
        self.levels = []
        for i, module in enumerate(net.pointnet_modules):
            plans = []
            for j, (grouper, mlp) in enumerate(zip(module.groupers, module.mlps)):
                use_xyz = bool(grouper.use_xyz)
                if module.n_points is None:
                    plans.append(("all", _GroupAllPlan(mlp, use_xyz)))
                elif _fusable(mlp, use_xyz, C, grouper.n_samples):
                    plans.append(("fused", _Fused(mlp, use_xyz, C, self.precision)))
                else:
                    plans.append(("module", self._copy((i, j), mlp)))
            self.levels.append(plans)
            C = sum(mlp.spec[-1] for mlp in module.mlps)

    def _encode(self, xyz, feature, sampling, lengths=None):
        """-> [(xyz, feature) after every set-abstraction level] (xyz None after the GroupAll level).  ``lengths``: only the first
        level's sampling reads them; the level kernels reach the cloud through idx, which never names a pad row."""
        net = self.net
        net.adopt_sampling(sampling)
        out = []
        for i, (module, plans) in enumerate(zip(net.pointnet_modules, self.levels)):
            s = sampling["levels"][i] if sampling is not None else (module.sample(xyz, lengths) if i == 0 else module.sample(xyz))
            xyz, feature = self._level(module, plans, xyz, feature, s)
            out.append((xyz, feature))
        return out

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


class FrozenPointNet2(_FrozenEncoder):
    """Frozen evaluator of ``PointNet2_cls`` / ``PointNetMSG`` (``frozen(net)``): the encoder plan of ``_FrozenEncoder``, then the
    eval-mode head kernels on at most 64 rows per call.  ``refresh()`` re-reads weights and running statistics from the network."""

    NET = PointNet2_cls

    @torch.no_grad()
    def refresh(self):
        self._refresh_encoder()
        self.head = self._copy("head", self.net.fc_layer)
        return self

    def __call__(self, xyz, feature, sampling=None, lengths=None):
        return self.run(xyz, feature, sampling, lengths)[1]

    @torch.no_grad()
    def run(self, xyz, feature, sampling=None, lengths=None):
        """-> ([feature of every set-abstraction level], logits [B, n_classes]).  ``lengths``: see ``frozen``."""
        lengths = self.net.resolve_lengths(xyz, sampling, lengths, self.net.pointnet_modules[0].n_points)
        feats = [f for _, f in self._encode(xyz, feature, sampling, lengths)]
        return feats, self._fc_head(feats[-1].squeeze(dim=1))


class _FusedFP(_SegStack):
    """Snapshot of one feature-propagation level for pcl_fp_level_infer_f32, optionally with the head layers behind it.

    ``D1`` skip channels (the first ``n_onehot`` of them the one-hot class label, a per-cloud bias), then the coarse
    channels; skips of at most 8 (other) channels fold inline, wider ones through the per-point table ``Us``."""

    def __init__(self, mlp, D1, n_onehot=0, head=()):
        layers = [(mlp, l, l < mlp.n_layers - 1 or mlp.last_act) for l in range(mlp.n_layers)]
        for h in head:
            layers += [(h, l, l < h.n_layers - 1 or h.last_act) for l in range(h.n_layers)]
        self.act_mask = sum(1 << i for i, (_, _, a) in enumerate(layers) if a)
        self.tap_layer = mlp.n_layers - 1 if head else None          # the level's own output, stored beside the head's
        super().__init__([(m, l) for m, l, _ in layers], first=None, pad_last=True)   # the last layer: padded to 32 columns
        W0 = self.W0
        self.D1, self.n_onehot, self.slope = D1, n_onehot, float(mlp.slope)
        self.CS = D1 - n_onehot
        self.inline = self.CS <= 8
        self.Woh = W0[:, :n_onehot].contiguous() if n_onehot else None
        self.Wsk = None if self.CS == 0 else (W0[:, n_onehot:D1] if self.inline else W0[:, n_onehot:D1].contiguous())
        self.Wc = W0[:, D1:].contiguous()

    @staticmethod
    def _rows(X, W, P=None):
        """X [P, Cin] W^T -> [P, Cout]: a product of the folded first layer (``_rows_gemm``, tagged ``pt``).  ``P`` is ``X.shape[0]``;
        tests/test_inference_partseg_gpu.py states it."""
        return _rows_gemm(X, W, tag="pt")

    def run(self, xyz1, xyz2, skip, coarse, onehot=None, lengths=None):
        """xyz1 [B,N,3], xyz2 [B,S,3], skip [B,N,D1 - n_onehot] (or None), coarse [B,S,D2], onehot [B, n_onehot]
        -> (out [B, N, widths[-1]], tap [B, N, widths[tap_layer]] or None).  ``lengths`` (device int32 [B]): the targets'
        per-cloud counts; rows beyond them come out as exact zeros."""
        B, N, _ = xyz1.shape
        S = coarse.shape[1]
        dev = xyz1.device
        Uc = self._rows(coarse.reshape(B * S, -1).contiguous(), self.Wc)
        idx3 = w3 = None
        if S == 1:                                                   # a one-row coarse level: a per-cloud bias
            cb, Uc = Uc, None
        else:
            idx3, w3 = three_nn(xyz1, xyz2, lengths1=lengths)
            cb = None
        if self.Woh is not None:
            c = self._rows(onehot.reshape(B, self.n_onehot).float().contiguous(), self.Woh)
            cb = c if cb is None else cb + c
        Us = fs = None
        if self.CS:
            fs = skip.reshape(B * N, self.CS).contiguous()
            if not self.inline:
                Us, fs = self._rows(fs, self.Wsk), None
        out = torch.empty((B, N, self.widths[-1]), dtype=torch.float32, device=dev)
        tap = None if self.tap_layer is None else torch.empty((B, N, self.widths[self.tap_layer]), dtype=torch.float32, device=dev)
        head = (_p(Us), _p(fs), _p(self.Wsk) if fs is not None else None, self.CS if fs is not None else 0, self.W0.shape[1], _p(Uc),
                _p(idx3), _p(w3), S, _p(cb))
        tail = (B, N, len(self.widths), self.c_widths, self.c_W, self.c_scale, self.c_shift, self.act_mask, self.slope, _p(out),
                out.shape[-1], _p(tap), -1 if tap is None else self.tap_layer, 0 if tap is None else tap.shape[-1], _stream())
        if lengths is None:
            _lib.call("pcl_fp_level_infer_f32", *head, *tail)
        else:
            _lib.call("pcl_fp_level_infer_ragged_f32", *head, _p(lengths), *tail)
        return out, tap


def _fp_supported(widths):
    return len(widths) <= 5 and bool(_lib.size_query("pcl_fp_level_infer_supported", len(widths), *(list(widths) + [0] * (5 - len(widths)))))


def _head_fusable(fp_mlp, head1, head2):
    """FP1 + Conv1d/BN (no activation) + Conv1d/bias (no BN, no activation) in one launch."""
    return (head1.n_layers == 1 and head2.n_layers == 1 and head1.bn and not head2.bn and not head1.last_act and not head2.last_act
            and head1.spec[0] == fp_mlp.spec[-1] and head2.spec[0] == head1.spec[-1]
            and _fp_supported([w.shape[0] for w in fp_mlp.weights] + [head1.spec[-1], head2.spec[-1]]))


class FrozenPointNet2Partseg(_FrozenEncoder):
    """Frozen evaluator of ``PointNet2_partseg`` / its ``PointNetMSG`` (``frozen(net)``): the encoder plan of the classifiers
    (``_FrozenEncoder``), one launch per feature-propagation level, the head fused into the last one.  ``refresh()`` re-reads
    weights and running statistics from the network.

    Each feature-propagation level runs the stats-free GEMMs of its folded first layer (``Uc = coarse W0c^T`` at the coarse
    resolution, ``Us = skip W0s^T`` per point, or the skip inline when it is narrow; the one-hot class label as a per-cloud bias)
    and then ONE ``pcl_fp_level_infer_f32`` launch.  The last level carries the head (Conv1d + BN, Dropout = identity, Conv1d) in
    the same launch, which also stores the level's own output (the tap).  FP levels and heads of other widths run eval-mode copies
    of their own modules."""

    NET = PointNet2_partseg
    N_ONEHOT = 16                 # FP1's skip: cat(one-hot class label [16], xyz [3], feature [3])  (pointnet2_partseg.py:170-173)

    @torch.no_grad()
    def refresh(self):
        net = self.net
        self._refresh_encoder()
        enc = [sum(mlp.spec[-1] for mlp in module.mlps) for module in net.pointnet_modules]
        skips = {"fp3": enc[1], "fp2": enc[0], "fp1": self.N_ONEHOT + 6}
        self.fp = {}
        for name in ("fp3", "fp2", "fp1"):
            mlp = getattr(net, name).mlp
            head = ()
            if name == "fp1" and _head_fusable(mlp, net.head1, net.head2):
                head = (net.head1, net.head2)
            widths = [w.shape[0] for w in mlp.weights] + [h.spec[-1] for h in head]
            if 2 <= mlp.n_layers and _fp_supported(widths):
                self.fp[name] = ("fused", _FusedFP(mlp, skips[name], self.N_ONEHOT if name == "fp1" else 0, head))
            else:
                self.fp[name] = ("module", self._copy(name, getattr(net, name)))
        self.head_fused = self.fp["fp1"][0] == "fused" and self.fp["fp1"][1].tap_layer is not None
        self.head = None if self.head_fused else (self._copy("head1", net.head1), self._copy("head2", net.head2))
        return self

    def __call__(self, xyz, feature, cls_label, sampling=None, lengths=None):
        return self.run(xyz, feature, cls_label, sampling, lengths)[1]

    @staticmethod
    def _zero_pads(t, lengths):
        """Exact zeros on the pad rows of t [B, N, C] (where, not a product: a pad row may hold NaN)."""
        valid = torch.arange(t.shape[1], device=t.device).view(1, -1) < lengths.view(-1, 1)
        return torch.where(valid.unsqueeze(-1), t, torch.zeros((), dtype=t.dtype, device=t.device))

    def _fp(self, name, xyz1, xyz2, skip, coarse, onehot=None, lengths=None):
        kind, plan = self.fp[name]
        if kind == "fused":
            return plan.run(xyz1, xyz2, skip, coarse, onehot, lengths)
        if onehot is not None:
            B, N, _ = xyz1.shape
            skip = torch.cat([onehot.view(B, 1, -1).expand(B, N, onehot.shape[-1]), skip], 2)
        if lengths is None:
            return plan(xyz1, xyz2, skip, coarse), None
        # the level's own module on a ragged batch: ragged 3-NN, then the eval-mode MLP (row-wise), then zeros on the pad rows
        B, N, _ = xyz1.shape
        if xyz2.shape[1] == 1:
            interp = coarse.expand(B, N, coarse.shape[2])
        else:
            idx3, w3 = three_nn(xyz1, xyz2, lengths1=lengths)
            interp = three_interpolate(coarse, idx3, w3)
        x = torch.cat([self._zero_pads(skip, lengths), interp], dim=-1) if skip is not None else interp
        return self._zero_pads(plan.mlp(x.contiguous()), lengths), None

    @torch.no_grad()
    def run(self, xyz, feature, cls_label, sampling=None, lengths=None):
        """-> ([sa1, sa2, sa3, fp3, fp2, fp1] level features, logits [B, part_num, N] (the network's layout and view)).
        ``lengths``: see ``frozen``; only FP1 (3-NN back onto the raw cloud, one row per raw point) sees them after level 1."""
        B, N, _ = xyz.shape
        xyz = xyz.contiguous()
        lengths = self.net.resolve_lengths(xyz, sampling, lengths, self.net.pointnet_modules[0].n_points)
        (l1_xyz, l1), (l2_xyz, l2), (_, l3) = self._encode(xyz, feature, sampling, lengths)
        l3_xyz = torch.zeros((B, 1, 3), device=xyz.device, dtype=xyz.dtype)
        f3, _ = self._fp("fp3", l2_xyz, l3_xyz, l2, l3)
        f2, _ = self._fp("fp2", l1_xyz, l2_xyz, l1, f3)
        onehot = cls_label.reshape(B, self.N_ONEHOT).float()
        out, tap = self._fp("fp1", xyz, l1_xyz, torch.cat([xyz, feature.float()], 2), f2, onehot, lengths)
        if self.head_fused:
            f1, logits = tap, out
        else:
            f1 = out
            h1, h2 = self.head
            logits = h2(h1(f1))
            if lengths is not None:                          # the head's bias / shift on FP1's zero pad rows
                logits = self._zero_pads(logits, lengths)
        return [l1, l2, l3, f3, f2, f1], logits.permute(0, 2, 1)


class FrozenPointNet(_Frozen):
    """Frozen evaluator of ``networks.cls.pointnet.PointNet``: ``fnet(x, lengths=None) -> [B, n_classes]`` for ``x`` [B, 3, N] (the
    network's input layout) of any strides -- a transposed view of a loader's [B, N, 3] is read as it is, no copy.  ``lengths``
    (``misc.ops._lengths``): per-cloud point counts of a ragged batch of capacity N; pad points may hold anything and every cloud's
    result is that of the cloud alone.  A device int32 tensor costs no host synchronisation and no packing.

    ``plan`` is ``"fused"`` when ``net.convs`` has the kernel's shape (3 -> 64/64/64/128/1024, BatchNorm, activation after every
    layer): dense weights, the eval constants of ``_eval_consts`` and the ctypes arrays are snapshot once, and a forward is
    ``pcl_pointnet_stack_infer_f32`` (csrc/infer_pointnet.hip: the five convs and the max over the points with the activations in
    LDS, nothing but per-tile maxima written) + the eval-mode head kernels (at most ``MAX_ROWS`` rows per call).  A stack of other
    widths gives ``"module"``: an eval-mode copy of ``net.convs`` runs, dense through ``group_max``, ragged through
    ``mlp_segment_max``.  ``refresh()`` re-reads weights and running statistics; ``net`` itself is never modified.

    ``precision``: "fp32", or "bf16" (``fnet.precision`` tells which) to run the fused stack as
    ``pcl_pointnet_stack_infer_bf16_f32``: layers 2-5 take bf16 operands (activations rounded to nearest even, weights snapshot as
    bf16 in ``refresh()``) and accumulate in fp32; layer 1, the epilogues, the max, the global feature and the head stay fp32
    (DESIGN.md section 21).  A ``"module"`` plan ignores the precision and stays fp32.

    The class is constructed directly; ``frozen(net)`` still takes the PointNet++ networks only (its tests pin that), and taking
    PointNet there is a later change."""

    NET = PointNet

    @torch.no_grad()
    def refresh(self):
        net, mlp = self.net, self.net.convs
        self._head = self._copy("head", torch.nn.Sequential(net.linear1, net.bn6, net.relu, net.dp1, net.linear2))
        self.head = list(self._head)
        L = len(mlp.weights)
        c_widths = (ctypes.c_int32 * L)(*[w.shape[0] for w in mlp.weights])
        C0 = mlp.weights[0].shape[1]
        fused = mlp.bn and mlp.last_act and bool(_lib.lib().pcl_pointnet_stack_infer_supported(C0, L, c_widths))
        self.plan = "fused" if fused else "module"
        if not fused:
            self._convs = self._copy("convs", mlp)
            return self
        self.slope = float(mlp.slope)
        bf16 = self.precision == "bf16"                                # layers 2-5 then take the stack's bf16 operands
        vars(self).update(vars(_SegStack([(mlp, l) for l in range(L)], bf16=bf16)))    # Ws, scales, shifts, c_*; bf16: Ws_bf16
        self.entry = _entry("pcl_pointnet_stack_infer_f32", self.precision)
        return self

    def __call__(self, x, lengths=None):
        return self.run(x, lengths)[1]

    def _stack(self, x, lengths):
        B, C0, N = x.shape
        if self.plan == "module":
            if lengths is None:
                return self._convs(x.transpose(1, 2).contiguous()[:, None], group_max=N).reshape(B, -1)
            lengths, row_off, R, row_cloud = packed_layout(lengths, B, N, x.device)
            return mlp_segment_max(self._convs, pack_rows(x.transpose(1, 2), lengths, row_off, R), row_off, row_cloud, B)
        self._require_f32_gpu(x)
        lengths = _lengths(lengths, B, N, x.device)
        width = self.widths[-1]
        ws_bytes = _lib.size_query("pcl_pointnet_stack_infer_workspace_bytes", B, N, width)
        ws = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=x.device)
        out = torch.empty((B, width), dtype=torch.float32, device=x.device)
        W0 = self.Ws[0]
        _lib.call(self.entry, _p(x), x.stride(0), x.stride(2), x.stride(1), _p(lengths), B, N, C0, _p(W0), W0.shape[1],
                  len(self.Ws), self.c_widths, self.c_W, self.c_scale, self.c_shift, self.slope, _p(ws), ws_bytes, _p(out), out.shape[1],
                  _stream())
        return out

    @torch.no_grad()
    def run(self, x, lengths=None):
        """-> (global feature [B, 1024], logits [B, n_classes])."""
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != self.net.convs.spec[0]:
            raise ValueError(f"FrozenPointNet: x must be [B,{self.net.convs.spec[0]},N], got {tuple(getattr(x, 'shape', ()))}")
        feature = self._stack(x, lengths)
        return feature, self._fc_head(feature)


# ---------------------------------------------------------------------------------------------- PointNet part segmentation
PARTSEG_CONCAT = (2048, 16, 64, 128, 128, 512, 2048)     # the head's input blocks: g | label | out1 | out2 | out3 | out4 | out5


def fold_partseg_head(Wh, W5, s5, t5, dtype=torch.float32):
    """The head's first weight ``Wh`` [C, 4944] (column blocks ``PARTSEG_CONCAT``) with ``out5 = s5 * (W5 out4) + t5`` folded away:
    -> (``Wrow`` [C, 832] on ``out1 | out2 | out3 | out4``, ``Wglob`` [C, 2064] on ``out_max | label``, ``c0`` [C]) with

        Wh . concat = Wrow . [out1|out2|out3|out4] + Wglob . [out_max|label] + c0,
        Wrow = [Wh_1 | Wh_2 | Wh_3 | Wh_4 + Wh_5 diag(s5) W5],  c0 = Wh_5 t5,  Wglob = [Wh_g | Wh_label].

    Formed in fp64 and rounded once to ``dtype``; plain torch, any device.  ``torch.bfloat16`` too is one rounding: torch casts
    fp64 to bf16 through fp32, which rounds twice, so the nearest bf16 value (ties to even) is taken in fp64 first."""
    g, lab, o1, o2, o3, o4, o5 = Wh.detach().double().split(list(PARTSEG_CONCAT), dim=1)
    W5, s5, t5 = W5.detach().double(), s5.detach().double(), t5.detach().double()
    Wrow = torch.cat([o1, o2, o3, o4 + (o5 * s5) @ W5], dim=1)

    def once(t):
        if dtype is torch.bfloat16:
            m, e = torch.frexp(t)                          # t = m * 2^e, 0.5 <= |m| < 1: 8 significant bits = round(m * 256)
            t = torch.ldexp(torch.round(m * 256.0), e - 8)
        return t.to(dtype).contiguous()

    return once(Wrow), once(torch.cat([g, lab], dim=1)), once(o5 @ t5)


def transposed_fc3(weight, bias, k):
    """A T-Net's last layer with its rows permuted and the identity added to the bias: ``(g @ W.T + b).reshape(k, k)`` is the
    TRANSPOSE of the module's ``(fc3(g) + I).reshape(k, k)`` -- the ``W[col][k]`` operand ``y = x @ T`` wants, with no transpose
    per forward.  -> (W [k*k, C], b [k*k]); plain torch, any device."""
    perm = torch.arange(k * k, device=weight.device).view(k, k).t().reshape(-1)
    b = bias.detach() + torch.eye(k, device=weight.device, dtype=bias.dtype).reshape(-1)      # the identity is symmetric
    return weight.detach()[perm].contiguous(), b[perm].contiguous()


def _seg_rows(x, W, scale, shift, slope, out=None):
    """``act(scale * (x W^T) + shift)`` on the B rows of x (pcl_pointnet_seg_rows_f32: a row's result does not depend on B)."""
    R, K = x.shape
    C = W.shape[0]
    if out is None:
        out = torch.empty((R, C), dtype=torch.float32, device=x.device)
    _lib.call("pcl_pointnet_seg_rows_f32", _p(x), x.stride(0), R, K, _p(W), C, _p(scale), _p(shift), float(slope), _p(out), out.stride(0),
              _stream())
    return out


class FrozenPointNetPartseg(_Frozen):
    """Frozen evaluator of ``networks.seg.pointnet_partseg.PointNet_partseg``: ``fnet(point_cloud, label, lengths=None) ->
    [B, part_num, N]`` for ``point_cloud`` [B, 3, N] of any strides and ``label`` [B, 16].  ``lengths`` (``misc.ops._lengths``):
    per-cloud point counts of a ragged batch of capacity N; pad points may hold anything, every cloud's result is bit for bit
    that of the cloud alone and the logits of pad points are exact zeros.  A device int32 tensor costs no host synchronisation.

    ``plan`` is ``"fused"`` when every stack has its kernel's shape (``pcl_pointnet_seg_infer_supported``; BatchNorm and the
    activation after every layer but ``conv5``'s, one slope): weights, eval constants, the folded head (``fold_partseg_head``)
    and the transposed ``fstn.fc3`` (``transposed_fc3``) are snapshot once, and a forward is the four launches of
    csrc/infer_pointnet_seg.hip with the B-row tails between them.  ``conv5`` has no activation, so the
    head's 4944-wide first layer folds to 832 columns on a row buffer ``out1 | out2 | out3 | out4`` plus a per-cloud bias
    (``fold_partseg_head``); neither the concatenation nor ``out5`` is ever stored.  Anything else gives ``"module"``: an eval-mode
    copy of the whole network runs (``forward``; ragged ``forward_packed`` scattered into zeros).  ``refresh()`` re-reads weights and
    running statistics; ``net`` itself is never modified.  Constructed directly: ``frozen()`` keeps its PointNet++ dispatch.

    ``precision``: "fp32", or "bf16" (``fnet.precision`` tells which) to run the two wide launches as
    ``pcl_pointnet_seg_global_infer_bf16_f32`` and ``pcl_pointnet_seg_head_infer_bf16_f32``: conv4, conv5 and the head's four layers
    take bf16 operands (activations rounded to nearest even) and accumulate in fp32; every weight of the two launches is snapshot
    as bf16 in ``refresh()``, the folded ``Wrow`` rounded once straight from fp64.  The two T-Net launches, the trunk, the product
    with ``T128``, the B-row tails, ``T3``, ``T128``, the row buffer, the epilogues, the max, the per-cloud bias and the logits stay
    fp32, a forward allocates what the fp32 forward does, and a ``"module"`` plan ignores the precision and stays fp32."""

    NET = PointNet_partseg
    N_LABEL = 16
    LDF = 832                      # row stride of the row buffer out1 | out2 | out3 | out4

    @staticmethod
    def _fusable(net):
        supported = _lib.lib().pcl_pointnet_seg_infer_supported
        convs = [net.conv1, net.conv2, net.conv3, net.conv4, net.conv5]
        mlps = [net.stn.convs, net.stn.fcs, net.fstn.convs, net.fstn.fcs, net.convs] + convs
        if not all(isinstance(m, PointwiseMLP) and m.bn for m in mlps) or any(c.n_layers != 1 for c in convs):
            return False
        if not all(m.last_act for m in mlps if m is not net.conv5) or net.conv5.last_act or len({m.slope for m in mlps}) != 1:
            return False
        if not all(isinstance(f, torch.nn.Linear) and f.bias is not None for f in (net.stn.fc3, net.fstn.fc3, net.convs4)):
            return False

        def ok(stack, spec):
            return bool(supported(_lib.define(stack), spec[0], len(spec) - 1, (ctypes.c_int32 * (len(spec) - 1))(*spec[1:])))

        trunk = [net.conv1.spec[0], net.conv1.spec[1], net.conv2.spec[1], net.conv3.spec[1]]
        chained = all(a.spec[-1] == b.spec[0] for a, b in zip(convs[:-1], convs[1:]))
        tails = all(t.k * t.k == t.fc3.out_features and t.fcs.spec[0] == t.convs.spec[-1] and t.fcs.spec[-1] == t.fc3.in_features
                    and all(c % 4 == 0 and c <= 2304 for c in t.fcs.spec) for t in (net.stn, net.fstn))
        return (chained and tails and net.stn.k == 3 and net.fstn.k == 128 and net.convs.spec[0] == sum(PARTSEG_CONCAT)
                and net.convs4.in_features == net.convs.spec[-1]
                and ok("PCL_SEG_STN", net.stn.convs.spec) and ok("PCL_SEG_TRUNK", trunk) and ok("PCL_SEG_FSTN", net.fstn.convs.spec)
                and ok("PCL_SEG_GLOBAL", [net.conv4.spec[0], net.conv4.spec[1], net.conv5.spec[1]])
                and ok("PCL_SEG_HEAD", [FrozenPointNetPartseg.LDF] + net.convs.spec[1:] + [net.convs4.out_features]))

    @staticmethod
    def _tail(tnet, fc3):
        """The B-row layers after a T-Net's max: [(W, scale | None, shift, slope)]"""
        fcs = tnet.fcs
        layers = []
        for l in range(fcs.n_layers):
            scale, shift = _eval_consts(fcs, l)
            layers.append((fcs.weights[l].detach().float().contiguous().clone(), scale, shift, float(fcs.slope)))
        return layers + [(fc3[0].float().contiguous().clone(), None, fc3[1].float().contiguous().clone(), 1.0)]

    @torch.no_grad()
    def refresh(self):
        net = self.net
        self.plan = "fused" if self._fusable(net) else "module"
        if self.plan == "module":
            self._module = self._copy("net", net)
            return self
        self.slope, self.part_num = float(net.conv1.slope), net.convs4.out_features
        self.stn = _SegStack([(net.stn.convs, l) for l in range(3)])
        self.trunk = _SegStack([(net.conv1, 0), (net.conv2, 0), (net.conv3, 0)])
        self.fstn = _SegStack([(net.fstn.convs, l) for l in range(3)])
        bf16 = self.precision == "bf16"                  # the global and head launches then take bf16 operands, all layers
        self.glob = _SegStack([(net.conv4, 0), (net.conv5, 0)], bf16=bf16, bf16_first=_OWN if bf16 else None)
        k3 = net.stn.k
        eye3 = torch.eye(k3, device=net.stn.fc3.bias.device, dtype=net.stn.fc3.bias.dtype).reshape(-1)
        self.stn_tail = self._tail(net.stn, (net.stn.fc3.weight.detach(), net.stn.fc3.bias.detach() + eye3))
        self.fstn_tail = self._tail(net.fstn, transposed_fc3(net.fstn.fc3.weight, net.fstn.fc3.bias, net.fstn.k))
        s5, t5 = self.glob.scales[1], self.glob.shifts[1]
        Wrow, self.Wglob, self.c0 = fold_partseg_head(net.convs.weights[0], net.conv5.weights[0], s5, t5)
        rows = -(-self.part_num // 32) * 32              # the last weight in whole 32-row blocks
        Wout = torch.zeros((rows, net.convs4.in_features), dtype=torch.float32, device=Wrow.device)
        Wout[:self.part_num] = net.convs4.weight.detach()
        self.bias_out = net.convs4.bias.detach().float().contiguous().clone()
        Wrow16 = None
        if bf16:                                         # fp64 -> bf16 in one rounding, not through the fp32 Wrow
            Wrow16 = fold_partseg_head(net.convs.weights[0], net.conv5.weights[0], s5, t5, dtype=torch.bfloat16)[0]
        self.head = _SegStack([(net.convs, l) for l in range(3)], first=Wrow, bf16=bf16, bf16_first=Wrow16)
        self.Wout = Wout
        self.head_widths = (ctypes.c_int32 * 4)(*self.head.widths, self.part_num)
        if bf16:
            Wout = self.Wout_bf16 = Wout.to(torch.bfloat16).contiguous()
        self.head_W = (ctypes.c_void_p * 4)(*[w.data_ptr() for w in self.head.operands + [Wout]])
        self.global_entry = _entry("pcl_pointnet_seg_global_infer_f32", self.precision)
        self.head_entry = _entry("pcl_pointnet_seg_head_infer_f32", self.precision)
        return self

    def __call__(self, point_cloud, label, lengths=None):
        return self.run(point_cloud, label, lengths)[3]

    @staticmethod
    def _run_tail(layers, g):
        for W, scale, shift, slope in layers:
            g = _seg_rows(g, W, scale, shift, slope)
        return g

    @torch.no_grad()
    def run(self, point_cloud, label, lengths=None):
        """-> (T3 [B,3,3], T128 [B,128,128], out_max [B,2048], logits [B, part_num, N]); the ``"module"`` plan returns None for the
        first three."""
        x = point_cloud
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != 3:
            raise ValueError(f"FrozenPointNetPartseg: point_cloud must be [B,3,N], got {tuple(getattr(x, 'shape', ()))}")
        B, _, N = x.shape
        if not isinstance(label, torch.Tensor) or tuple(label.shape) != (B, self.N_LABEL):
            raise ValueError(f"FrozenPointNetPartseg: label must be [{B},{self.N_LABEL}], got {tuple(getattr(label, 'shape', ()))}")
        if self.plan == "module":
            if lengths is None:
                return None, None, None, self._module(x, label)
            rows, row_off = self._module.forward_packed(x, label, lengths)
            lengths = _lengths(lengths, B, N, x.device)
            return None, None, None, unpack_rows(rows, lengths, row_off, N).permute(0, 2, 1)
        self._require_f32_gpu(x, "point cloud")
        if label.device != x.device or label.dtype != torch.float32:
            raise TypeError(f"FrozenPointNetPartseg: label must be float32 on {x.device}, got {label.dtype} on {label.device}")
        dev, st = x.device, _stream()
        lengths = _lengths(lengths, B, N, dev)
        ws_bytes = _lib.size_query("pcl_pointnet_seg_part_workspace_bytes", B, N, 2048)
        f_bytes = _lib.size_query("pcl_pointnet_seg_rows_workspace_bytes", B, N, self.LDF)
        ws = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=dev)
        F = torch.empty((f_bytes // 4,), dtype=torch.float32, device=dev)
        strides = (x.stride(0), x.stride(2), x.stride(1))
        s = self.stn
        g = torch.empty((B, 1024), dtype=torch.float32, device=dev)
        _lib.call("pcl_pointnet_seg_stn_infer_f32", _p(x), *strides, _p(lengths), B, N, s.L, s.c_widths, _p(s.Ws[0]), 3, s.c_W, s.c_scale,
                  s.c_shift, self.slope, _p(ws), ws_bytes, _p(g), 1024, st)
        T3 = self._run_tail(self.stn_tail, g)
        c, s = self.trunk, self.fstn
        g = torch.empty((B, 1024), dtype=torch.float32, device=dev)
        _lib.call("pcl_pointnet_seg_trunk_infer_f32", _p(x), *strides, _p(lengths), B, N, _p(T3), c.L, c.c_widths, _p(c.Ws[0]), 3, c.c_W,
                  c.c_scale, c.c_shift, s.L, s.c_widths, s.c_W, s.c_scale, s.c_shift, self.slope, _p(F), self.LDF, f_bytes, _p(ws),
                  ws_bytes, _p(g), 1024, st)
        TT = self._run_tail(self.fstn_tail, g)
        c = self.glob
        glob = torch.empty((B, 2048 + self.N_LABEL), dtype=torch.float32, device=dev)      # out_max | label
        glob[:, 2048:] = label
        _lib.call(self.global_entry, _p(F), self.LDF, f_bytes, _p(lengths), B, N, _p(TT), c.L, c.c_widths, c.c_W,
                  c.c_scale, c.c_shift, self.slope, _p(ws), ws_bytes, _p(glob), glob.stride(0), st)
        bias = _seg_rows(glob, self.Wglob, None, self.c0, 1.0)
        h = self.head
        out = torch.empty((B, self.part_num, N), dtype=torch.float32, device=dev)
        _lib.call(self.head_entry, _p(F), self.LDF, f_bytes, _p(lengths), B, N, _p(bias), bias.stride(0), 4,
                  self.head_widths, self.head_W, self.Wout.shape[0], h.c_scale, h.c_shift, _p(self.bias_out), self.slope, _p(out),
                  out.stride(0), out.stride(1), out.stride(2), st)
        return T3.view(B, 3, 3), TT.view(B, 128, 128).transpose(1, 2), glob[:, :2048], out


# ---------------------------------------------------------------------------------------------- PointConv classification
POINTCONV_M = 16                                         # WeightNet(3, 16)


def pack_small_nets(weightnet, densitynet):
    """The eval constants of a level's WeightNet (3 -> 8 -> 8 -> 16) and DensityNet (1 -> 8 -> 8 -> 1) as the one packed buffer of
    ``PCL_POINTCONV_NETS_FLOATS`` floats ``pcl_pointconv_level_infer_f32`` takes: per net and layer the dense weight ``[out][in]``,
    then the folded ``scale`` and ``shift`` (``_eval_consts``), at the offsets include/pcl_hip.h lists.  Plain torch, any device."""
    parts = []
    for mlp in (weightnet.mlp, densitynet.mlp):
        for l in range(mlp.n_layers):
            parts += [mlp.weights[l].detach().float().reshape(-1), *_eval_consts(mlp, l)]
    flat = torch.cat(parts)
    out = torch.zeros(_lib.define("PCL_POINTCONV_NETS_FLOATS"), dtype=torch.float32, device=flat.device)
    out[:flat.numel()] = flat
    return out


class _LevelLinear:
    """Snapshot of a level's ``Linear(16 C -> C)`` + BatchNorm1d + ReLU (a one-layer PointwiseMLP): the stats-free GEMM of the family
    ``_linear_flush`` selects for the call's shape under ``net.eval()`` (bias in the GEMM, as there), then ``pcl_bn_act_f32`` with the
    eval constants."""

    def __init__(self, mlp):
        self.W = mlp.weights[0].detach().float().contiguous().clone()
        self.bias = None if mlp.biases is None else mlp.biases[0].detach().float().contiguous().clone()
        self.scale, self.shift = _eval_consts(mlp, 0, fold_bias=False)
        self.slope = float(mlp.slope) if mlp.last_act else 1.0

    def run(self, X):
        P, K = X.shape
        C = self.W.shape[0]
        st = _stream()
        flush = _linear_flush(K, P)
        if flush:
            Y = torch.empty((P, C), dtype=torch.float32, device=X.device)
            _lib.call("pcl_frag_linear_fwd_f32", _p(X), K, _p(self.W), K, _p(self.bias), None, None, 0.0, P, K, C, _p(Y), C, None, None,
                      flush, st, tag=f"fwd{K}x{C}")
        else:
            Y = _rows_gemm(X, self.W, self.bias)
        out = torch.empty_like(Y)
        _lib.call("pcl_bn_act_f32", _p(Y), _p(self.scale), _p(self.shift), self.slope, P, C, _p(out), st)
        return out


def _small_nets_ok(sa):
    wn, dn = sa.weightnet, sa.densitynet
    return (isinstance(wn, WeightNet) and isinstance(dn, DensityNet) and wn.mlp.spec == [3, 8, 8, POINTCONV_M] and dn.mlp.spec == [1, 8, 8, 1]
            and all(m.bn and m.last_act and m.slope == 0.0 for m in (wn.mlp, dn.mlp))
            and sa.linear.n_layers == 1 and sa.linear.bn)


def _pointconv_fusable(sa, D):
    mlp = sa.mlp
    if sa.group_all or not (mlp.n_layers == 3 and mlp.bn and mlp.last_act and mlp.spec[0] == 3 + D and _small_nets_ok(sa)):
        return False
    return bool(_lib.size_query("pcl_pointconv_level_infer_supported", int(sa.nsample), 3, *[int(c) for c in mlp.spec[1:]], POINTCONV_M))


class _FusedPointConv(_SegStack):
    """Snapshot of one k-NN PointConv level for pcl_pointconv_level_infer_f32 (or, ``precision="bf16"``,
    pcl_pointconv_level_infer_bf16_f32): the feature MLP (first layer folded), the packed small nets and the level's Linear.
    ``entry``: the fp32 name of another entry point of the same argument list (pcl_pointconv_seg_level_infer_f32: feature MLPs of
    2 or 3 layers)."""

    def __init__(self, sa, D, precision="fp32", entry="pcl_pointconv_level_infer_f32"):
        mlp = sa.mlp
        super().__init__([(mlp, l) for l in range(mlp.n_layers)], first=None, bf16=precision == "bf16")
        self.precision = precision
        self.entry = _entry(entry, precision)
        self.D, self.slope = D, float(mlp.slope)
        self.ldw = self.W0.shape[1]                                    # Wx = W0[:, :3]: the kernel reads it with the row stride ldw
        self.Wf = self.W0[:, 3:].contiguous() if D else None
        self.nets = pack_small_nets(sa.weightnet, sa.densitynet)
        self.linear = _LevelLinear(sa.linear)

    def contract(self, xyz, new_xyz, points, idx, density):
        """-> the contraction output [B*S, 16 C3] (the level up to misc/pointconv_utils.py:394)."""
        B, N, _ = xyz.shape
        S, ns = idx.shape[1], idx.shape[2]
        C1, C3 = self.widths[0], self.widths[-1]
        Uf = _rows_gemm(points.reshape(B * N, self.D), self.Wf, tag="pt") if self.D else None
        out = torch.empty((B * S, POINTCONV_M * C3), dtype=torch.float32, device=xyz.device)
        if any(t is not None and t.data_ptr() % 16 for t in (Uf, out, *self.operands[1:])):      # the entry point's precondition (pcl_hip.h)
            raise ValueError(f"{self.entry}: Uf, the weights and out must be 16-byte aligned")
        rows = B * S * ns
        _lib.call(self.entry, _p(xyz), _p(new_xyz), _p(Uf), _p(self.W0), self.ldw, _p(density), _p(idx), B, N, S, ns, self.L,
                  self.c_widths, self.c_W, self.c_scale, self.c_shift, self.slope, _p(self.nets), POINTCONV_M, _p(out), out.shape[1],
                  _stream(), algo_flops=2 * rows * (3 * C1 + sum(a * b for a, b in zip(self.widths, self.widths[1:])) + POINTCONV_M * C3 + 296),
                  tag=f"pointconv{ns}x{C3}" if self.L == 3 else f"pointconv{ns}x{C3}L{self.L}")
        return out

    def run(self, xyz, new_xyz, points, idx, density):
        B, S = idx.shape[0], idx.shape[1]
        return self.linear.run(self.contract(xyz, new_xyz, points, idx, density)).view(B, S, -1)


class _PointConvGroupAll:
    """Snapshot of the ``group_all`` level: the feature MLP, the WeightNet and the DensityNet as stats-free GEMM chains
    (``_RowsStack``), ``pcl_pointconv_contract_bn_f32`` with the feature MLP's last eval constants, and an eval-mode copy of the
    level's Linear (16384 -> 1024 on B rows: the wide head kernels ``net.eval()`` uses)."""

    def __init__(self, sa, linear):
        self.feat, self.weightnet, self.densitynet = _RowsStack(sa.mlp), _RowsStack(sa.weightnet.mlp), _RowsStack(sa.densitynet.mlp)
        self.linear = linear

    def run(self, xyz, points, density):
        B, N, _ = xyz.shape
        P = B * N
        local = xyz - xyz.mean(dim=1, keepdim=True)                    # sample_and_group_all: relative to the centroid
        rows = (torch.cat([local, points], dim=-1) if points is not None else local).reshape(P, -1).contiguous()
        Y, sc, sh = self.feat.run(rows)
        C = Y.shape[1]
        weights = self.weightnet.run_act(local.reshape(P, 3))
        rho = self.densitynet.run_act(density.reshape(P, 1))
        out = torch.empty((B, C * POINTCONV_M), dtype=torch.float32, device=xyz.device)
        _lib.call("pcl_pointconv_contract_bn_f32", _p(Y), _p(sc), _p(sh), self.feat.out_slope, _p(rho), _p(weights), B, N, C, POINTCONV_M,
                  _p(out), _stream())
        return _pointconv_linear(self.linear, out.view(B, 1, -1))


class FrozenPointConv(_Frozen):
    """Frozen evaluator of ``networks.cls.pointconv.PointConvDensityClsSsg``: ``fnet(xyz [B,3,N], start_idx=None, knn_lists=None,
    sampling=None) -> [B, n_classes]``, the signature of ``net.forward``; ``fnet.run(...)`` also returns the three level features
    (channel-last: ``[B, S, C]``).  Index lists and densities come from the network's own ``sa.sample`` (or a handle of
    ``net.precompute_sampling``).  Constructed directly.

    ``fnet.levels`` names the plan per level.  ``"fused"`` for a k-NN level whose shape has a kernel
    (``pcl_pointconv_level_infer_supported``; csrc/infer_pointconv.hip): the per-point product ``Uf = points
    W0[:, 3:]^T`` (stats-free library GEMM), then ONE ``pcl_pointconv_level_infer_f32`` launch that runs the feature MLP, the
    WeightNet and the DensityNet of every row and the density-weighted contraction with its activations in LDS -- the ``[B*S, 16
    C]`` contraction output is the only large tensor a level writes -- then the level's ``Linear(16 C -> C)`` as a stats-free GEMM of
    the family ``net.eval()`` selects, with the eval constants.  ``"all"`` for a ``group_all`` level of the usual small nets: the
    stats-free GEMMs and ``pcl_pointconv_contract_bn_f32``.  ``"module"`` otherwise -- an eval-mode copy of the level's own module
    runs.  The head runs the eval-mode head kernels.  ``refresh()`` re-reads weights and running statistics; ``net`` itself is
    never modified (parameters, buffers, ``training`` flags).

    ``precision``: "fp32", or "bf16" (``fnet.precision`` tells which) to run every fused level launch as
    ``pcl_pointconv_level_infer_bf16_f32``: layers 2 and 3 of the feature MLP take bf16 operands (activations rounded to nearest
    even, weights snapshot as bf16 in ``refresh()``) and accumulate in fp32; ``Uf``, layer 1, the WeightNet, the DensityNet, the
    epilogues, ``z3``, the contraction and its output stay fp32, and so do the level's Linear, the ``group_all`` level, ``"module"``
    fallbacks and the head.  ``levels`` does not depend on it, and everything but the fused launches is the same code on the same
    types."""

    NET = PointConvDensityClsSsg

    @torch.no_grad()
    def refresh(self):
        net = self.net
        self.plans = []
        D = 0
        for name in ("sa1", "sa2", "sa3"):
            sa = getattr(net, name)
            if isinstance(sa, PointConvDensitySetAbstraction) and _pointconv_fusable(sa, D):
                self.plans.append(("fused", _FusedPointConv(sa, D, self.precision)))
            elif (isinstance(sa, PointConvDensitySetAbstraction) and sa.group_all and sa.mlp.bn and sa.mlp.last_act and sa.mlp.spec[0] == 3 + D
                  and _small_nets_ok(sa)):
                self.plans.append(("all", _PointConvGroupAll(sa, self._copy((name, "linear"), sa.linear))))
            else:
                self.plans.append(("module", self._copy(name, sa)))
            D = sa.linear.spec[-1]
        self.levels = [k for k, _ in self.plans]
        self._head = self._copy("head", torch.nn.Sequential(net.fc1, net.bn1, net.relu, net.drop1, net.fc2, net.bn2, net.relu, net.drop2, net.fc3))
        self.head = list(self._head)
        return self

    def __call__(self, xyz, start_idx=None, knn_lists=None, sampling=None):
        return self.run(xyz, start_idx, knn_lists, sampling)[1]

    @staticmethod
    def _sample(sa, xyz, start_idx, knn_idx):
        if knn_idx is None or sa.group_all:
            return sa.sample(xyz, start_idx)
        new_xyz, idx = sample_level(sa.npoint, sa.nsample, xyz, start_idx, knn_idx)
        return new_xyz, [(idx, compute_density(xyz, sa.bandwidth))]

    @torch.no_grad()
    def run(self, xyz, start_idx=None, knn_lists=None, sampling=None):
        """-> ([feature of sa1, sa2, sa3: [B, S, C]], logits [B, n_classes])."""
        if not isinstance(xyz, torch.Tensor) or xyz.dim() != 3 or xyz.shape[1] != 3:
            raise ValueError(f"FrozenPointConv: xyz must be [B,3,N], got {tuple(getattr(xyz, 'shape', ()))}")
        self._require_f32_gpu(xyz)
        net = self.net
        B = xyz.shape[0]
        SamplingPrefetch.adopt_sampling(sampling)
        knn = (None, None, None) if knn_lists is None else (*knn_lists, None)
        starts = (None, None, None) if start_idx is None else (start_idx[0], start_idx[1], None)
        pts = xyz.permute(0, 2, 1).contiguous()
        points = None
        feats = []
        for i, (name, (kind, plan)) in enumerate(zip(("sa1", "sa2", "sa3"), self.plans)):
            sa = getattr(net, name)
            lv = sampling["levels"][i] if sampling is not None else self._sample(sa, pts, starts[i], knn[i])
            new_xyz, ((idx, density),) = lv
            if kind == "fused":
                points = plan.run(pts, new_xyz.contiguous(), points, idx.contiguous(), density.contiguous())
            elif kind == "all":
                points = plan.run(pts, points, density.contiguous())
            else:
                nx, f = plan(pts.permute(0, 2, 1), None if points is None else points.permute(0, 2, 1), sampling=lv)
                points = f.permute(0, 2, 1).contiguous()
                if new_xyz is None:
                    new_xyz = nx.permute(0, 2, 1)
            feats.append(points)
            pts = new_xyz.contiguous() if new_xyz is not None else None
        return feats, self._fc_head(feats[-1].reshape(B, -1))


# ---------------------------------------------------------------------------------------------- PointConv part segmentation
def _pointconv_seg_fusable(level, D, query="pcl_pointconv_seg_level_infer_supported"):
    """A k-NN level (set abstraction or interpolation) of the usual small nets whose shape ``pcl_pointconv_seg_level_infer_f32``
    has a kernel for (or, by its ``query``, ``pcl_pointconv_wide_level_infer_f32``).  In the query C2 = widths[1] and C3 =
    widths[L-1] (include/pcl_hip.h)."""
    mlp = level.mlp
    if getattr(level, "group_all", False) or not (mlp.n_layers in (2, 3) and mlp.bn and mlp.last_act and mlp.spec[0] == 3 + D
                                                   and _small_nets_ok(level)):
        return False
    w = [int(c) for c in mlp.spec[1:]]
    return bool(_lib.size_query(query, int(level.nsample), len(w), w[0], w[1], w[-1], POINTCONV_M))


class FrozenPointConvPartseg(_Frozen):
    """Frozen evaluator of ``networks.seg.pointconv_partseg.PointConvDensity_partseg``: ``fnet(xyz [B,N,3], cls_label=None,
    sampling=None, start_idx=None) -> [B, N, part_num]``, the signature and layout of ``net.forward`` (``cls_label`` is accepted
    and unused, as there); ``fnet.run(...)`` also returns the eight level outputs (channel-last ``[B, S, C]``, in call order
    ``sa0..sa3, in0..in3``; an interpolation level's rows are in its FPS visiting order, as upstream).  ``sampling``: a handle of
    ``net.precompute_sampling(xyz)``; without one the evaluator calls it with ``start_idx`` (eight [B] int32 FPS starts, or None
    for random ones).  Constructed directly.

    ``fnet.levels`` names the plan per level.  The eight levels are k-NN levels, and each one whose
    (neighbours, widths) have a kernel (``pcl_pointconv_seg_level_infer_supported``: feature MLPs of two or three layers, 16 or 32
    neighbours) is ``"fused"``: ONE ``pcl_pointconv_seg_level_infer_f32`` launch plus its Linear, as in ``FrozenPointConv``.  An
    interpolation level first runs the 3-NN interpolation and ``Uf = interpolated W0[:, 3:]^T`` over its N points, then that launch
    over N groups of 16 (the centres are the level's own points in FPS visiting order, as upstream), so no ``[B,N,16,C]`` tensor
    exists.  ``"module"`` otherwise -- an eval-mode copy of the level's own module runs on the same sampling entry: the two 512-wide
    levels (``sa3``, ``in0``) have no kernel in that table (``wide_levels``, below).  The head runs the stats-free GEMMs on the ``B N`` rows.  ``refresh()`` re-reads
    weights and running statistics; ``net`` itself is never modified (parameters, buffers, ``training`` flags).

    ``precision``: "fp32", or "bf16" (``fnet.precision`` tells which) to run every fused level launch as
    ``pcl_pointconv_seg_level_infer_bf16_f32``: the layers behind the first of the feature MLP (one at two layers, two at three)
    take bf16 operands (activations rounded to nearest even, weights snapshot as bf16 in ``refresh()``) and accumulate in fp32;
    ``Uf``, layer 1, the WeightNet, the DensityNet, the epilogues, the last activation, the contraction and its output stay fp32.
    ``levels`` does not depend on it, and everything but the fused launches -- the 3-NN interpolation, ``Uf``, each level's Linear,
    the two ``"module"`` levels, the head -- is the same code on the same types.

    ``wide_levels``: False, or True (``fnet.wide_levels`` tells which) to run a level that the table above
    rejects and ``pcl_pointconv_wide_level_infer_supported`` accepts -- ``sa3`` (32 neighbours, 256/256/512) and ``in0`` (16
    neighbours, 512/512) of the stock network -- as ``"fused"`` too: ``Uf``, ONE ``pcl_pointconv_wide_level_infer_f32`` launch (the
    same values, the last layer and the contraction a chunk of columns at a time, one workgroup per compute unit), then its Linear,
    exactly as the six others; ``in0`` runs the 3-NN interpolation first.  The stock network is then ``["fused"] * 8`` and a forward
    forms no BatchNorm constants and no ``[B,S,ns,C]`` tensor.  The wide kernel is fp32 only: under ``precision="bf16"`` those
    levels run the fp32 wide kernel, so ``levels`` does not depend on the precision here either.  With False (the default) plans,
    launches and bits are what they were.  What it saves is the two module copies' small launches and grouped tensors; each
    level's 8192 -> 512 Linear is untouched and is the larger part of what those two levels still cost (DESIGN.md section 28 has
    the measured times)."""

    NET = PointConvDensity_partseg
    WIDE_ENTRY = "pcl_pointconv_wide_level_infer_f32"

    def __init__(self, net, precision="fp32", wide_levels=False):
        if not isinstance(wide_levels, bool):
            raise ValueError(f"FrozenPointConvPartseg: wide_levels must be a bool, got {wide_levels!r}")
        self.wide_levels = wide_levels
        super().__init__(net, precision)

    @torch.no_grad()
    def refresh(self):
        net = self.net
        self.plans = []
        D = 0
        for name in net.LEVELS:
            level = getattr(net, name)
            kinds = (PointConvDensitySetAbstraction, PointConvDensitySetInterpolation)
            if isinstance(level, kinds[1]):
                D = level.mlp.spec[0] - 3                              # the interpolated features of the level below
            if isinstance(level, kinds) and _pointconv_seg_fusable(level, D):
                self.plans.append(("fused", _FusedPointConv(level, D, self.precision, entry="pcl_pointconv_seg_level_infer_f32")))
            elif self.wide_levels and isinstance(level, kinds) and _pointconv_seg_fusable(level, D, "pcl_pointconv_wide_level_infer_supported"):
                self.plans.append(("fused", _FusedPointConv(level, D, "fp32", entry=self.WIDE_ENTRY)))   # fp32 under either precision
            else:
                self.plans.append(("module", self._copy(name, level)))
            D = level.linear.spec[-1]
        self.levels = [k for k, _ in self.plans]
        fc1, fc3 = net.fc1, net.fc3
        self.fc1 = _RowsStack(fc1)
        self.W3 = fc3.weight.detach().float().contiguous().clone()
        self.b3 = None if fc3.bias is None else fc3.bias.detach().float().contiguous().clone()
        return self

    def __call__(self, xyz, cls_label=None, sampling=None, start_idx=None):
        return self.run(xyz, cls_label, sampling, start_idx)[1]

    def _head(self, rows):
        """fc1 + bn1 + relu (Dropout = identity), fc3: fc1's BatchNorm + activation ride in fc3's operand load."""
        Y, sc, sh = self.fc1.run(rows)
        return _rows_gemm(Y, self.W3, self.b3, sc, sh, self.fc1.out_slope)

    @torch.no_grad()
    def run(self, xyz, cls_label=None, sampling=None, start_idx=None):
        """-> ([output of sa0..sa3, in0..in3: [B, S, C]], logits [B, N, part_num])."""
        if not isinstance(xyz, torch.Tensor) or xyz.dim() != 3 or xyz.shape[2] != 3:
            raise ValueError(f"FrozenPointConvPartseg: xyz must be [B,N,3], got {tuple(getattr(xyz, 'shape', ()))}")
        self._require_f32_gpu(xyz)
        B, N, _ = xyz.shape
        if sampling is None:
            sampling = self.net.precompute_sampling(xyz, start_idx)
        levels = sampling["levels"]
        pts, feats, points = [xyz.contiguous()], [], None
        for i in range(4):
            points = self._level(i, pts[-1], None, points, levels[i])
            feats.append(points)
            pts.append(levels[i][0].contiguous())
        for k in range(4):                                             # in_k reads the coordinates of levels 3 - k and 4 - k
            points = self._level(4 + k, pts[3 - k], pts[4 - k], points, levels[4 + k])
            feats.append(points)
        return feats, self._head(points.reshape(B * N, -1)).view(B, N, -1)

    def _level(self, i, xyz1, xyz2, points, lv):
        """Level ``i`` (call order) on its sampling entry ``lv``, channel-last: a set-abstraction level on (xyz1, points), an
        interpolation level on (xyz1, xyz2, points of xyz2) -> the level's output [B, S, C]."""
        kind, plan = self.plans[i]
        cf = lambda t: t.permute(0, 2, 1)                              # channel-last <-> channel-first, for the module copies
        if i < 4:
            new_xyz, ((idx, density),) = lv
            if kind == "fused":
                return plan.run(xyz1, new_xyz.contiguous(), points, idx.contiguous(), density.contiguous())
            return cf(plan(cf(xyz1), None if points is None else cf(points), sampling=lv)[1]).contiguous()
        if kind == "fused":
            interpolated = three_interpolate(points.contiguous(), lv["idx3"], lv["w3"])
            return plan.run(xyz1, lv["new_xyz"].contiguous(), interpolated, lv["idx"].contiguous(), lv["density"].contiguous())
        return cf(plan(cf(xyz1), cf(xyz2), None, cf(points), sampling=lv)).contiguous()


# ---------------------------------------------------------------------------------------------- PointCNN classification
def _bn_last_consts64(bn):
    """(scale, shift) in fp64 of a ``_BatchNormLast`` in evaluation mode."""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return s, bn.bias.detach().double() - s * bn.running_mean.double()


def _consts64(mlp, l):
    """``_eval_consts(mlp, l)`` in fp64: (W, scale, shift) with the conv bias folded into the shift."""
    W = mlp.weights[l].detach().double()
    bias = None if mlp.biases is None else mlp.biases[l].detach().double()
    if mlp.bn:
        rm, rv = getattr(mlp, f"running_mean_{l}").double(), getattr(mlp, f"running_var_{l}").double()
        scale = mlp.gammas[l].detach().double() / torch.sqrt(rv + mlp.eps)
        shift = mlp.betas[l].detach().double() - scale * (rm if bias is None else rm - bias)
    else:
        scale = torch.ones(W.shape[0], dtype=torch.float64, device=W.device)
        shift = torch.zeros_like(scale) if bias is None else bias
    return W, scale, shift


def fold_affine_into_linear(W, b, s, t):
    """``W (s * z + t) + b = (W diag(s)) z + (W t + b)`` in fp64: the affine map in FRONT of a Linear folded into its weight and
    bias -> (W', b').  A stage of PointCNN ends ``s * relu(raw) + t`` (``SepConv`` activates, then normalises), and what reads it is
    linear: the next stage's ``dense`` and the head's first layer."""
    W = W.detach().double()
    return W * s.double().unsqueeze(0), W @ t.double() + (0 if b is None else b.detach().double())


def fold_xtrans(xc):
    """The X-transform of an ``XConv`` in evaluation mode with ``x_trans_0``'s trailing BatchNorm folded into ``x_trans_1``, in
    fp64: ``x0 = relu(W0 p)``, ``x1 = relu(sc1 * (W1 x0) + sh1)``, ``X = W2 x1 + b2`` -> (W0, W1, sc1, sh1, W2, b2).  ``x_trans_0``
    is Linear, ReLU, THEN the affine (s0, t0), so ``W1 = W1' diag(s0)`` and ``sh1 = shift1' + scale1' * (W1' t0)``."""
    s0, t0 = _bn_last_consts64(xc.x_trans_0.bn)
    W0 = xc.x_trans_0.linear.weights[0].detach().double()
    W1, sc1, sh1 = _consts64(xc.x_trans_1.mlp, 0)
    W2, _, b2 = _consts64(xc.x_trans_2.mlp, 0)
    return W0, W1 * s0.unsqueeze(0), sc1, sh1 + sc1 * (W1 @ t0), W2, b2


def _pad_to16(W):
    """[R, C] with both dimensions that are no multiple of 16 padded to one with zeros (rows only where ``R`` is not)."""
    r, c = (-(-n // 16) * 16 for n in W.shape)
    out = torch.zeros((r, c), dtype=W.dtype, device=W.device)
    out[:W.shape[0], :W.shape[1]] = W
    return out


def _relu_mlp(mlp, layers, bn=True, act=True):
    return (isinstance(mlp, PointwiseMLP) and mlp.n_layers == layers and bool(mlp.bn) == bn and bool(mlp.last_act) == act
            and mlp.slope == 0.0)


def _xconv_fusable(stage):
    """A ``RandPointCNN`` of the usual parts (per-point dense, ReLU everywhere, BatchNorm where the stock modules have one) whose
    shape ``pcl_xconv_level_infer_f32`` has a kernel for."""
    if not isinstance(stage, RandPointCNN) or not _xconv_stock_parts(stage.pointcnn):
        return False
    pc, xc = stage.pointcnn, stage.pointcnn.x_conv
    return bool(_lib.size_query("pcl_xconv_level_infer_supported", int(pc.K), int(xc.C_mid), int(xc.C_in), int(xc.end_conv.dm)))


def _xconv_stock_parts(pc):
    """A ``PointCNN`` of the usual parts: per-point dense, ReLU everywhere, BatchNorm where the stock modules have one."""
    if pc.dense is None:
        return False
    xc = pc.x_conv
    ec = xc.end_conv
    return (xc.dims == 3 and _relu_mlp(pc.dense.mlp, 1) and _relu_mlp(xc.dense, 2) and _relu_mlp(xc.x_trans_0.linear, 1, bn=False)
            and xc.x_trans_0.bn is not None and _relu_mlp(xc.x_trans_1.mlp, 1) and _relu_mlp(xc.x_trans_2.mlp, 1, bn=False, act=False)
            and ec.backend == "auto" and ec.bn is not None and _relu_mlp(ec.pointwise, 1, bn=False) and pc.dense.mlp.biases is not None)


class _FusedXConv:
    """Snapshot of one X-conv stage for ``pcl_xconv_level_infer_f32``: the per-point dense (with the affine of the stage below
    folded in, ``in_affine`` = its (s, t) in fp64 or None for plain input rows), the lift, the folded X-transform, the depthwise
    taps and the pointwise weight; ``out_affine``: the (s, t) of this stage's own trailing BatchNorm, for whoever reads ``raw``."""

    def __init__(self, stage, in_affine):
        pc, xc = stage.pointcnn, stage.pointcnn.x_conv
        ec = xc.end_conv
        f32 = lambda t: t.detach().float().contiguous().clone()
        self.K, self.D, self.P, self.C_mid, self.C2, self.dm = int(pc.K), int(pc.D), int(stage.P), int(xc.C_mid), int(xc.C_in), int(ec.dm)
        dense = pc.dense.mlp
        self.folded = in_affine is not None
        if self.folded:
            Wd, bd = fold_affine_into_linear(dense.weights[0], dense.biases[0], *in_affine)
            dev = Wd.device
            self.ones, self.zeros = torch.ones(Wd.shape[1], device=dev), torch.zeros(Wd.shape[1], device=dev)
        else:
            Wd, bd = dense.weights[0], dense.biases[0]
        self.Wd, self.bd = f32(Wd), f32(bd)
        self.fs, self.ft = _eval_consts(dense, 0, fold_bias=False)
        lift = xc.dense
        self.Wa, self.Wb = f32(lift.weights[0]), _pad_to16(f32(lift.weights[1]))
        (self.sa, self.ta), (self.sb, self.tb) = _eval_consts(lift, 0), _eval_consts(lift, 1)
        W0, W1, sc1, sh1, W2, b2 = fold_xtrans(xc)
        self.W0 = _pad_to16(f32(W0))                                   # [K*K, 3K] -> 3K padded to a multiple of 16
        self.W1, self.sc1, self.sh1, self.W2, self.b2 = f32(W1), f32(sc1), f32(sh1), f32(W2), f32(b2)
        self.wd, self.bias = f32(ec.depthwise), f32(ec.depthwise_bias)
        self.Wp = f32(ec.pointwise.weights[0])
        self.out_affine = _bn_last_consts64(ec.bn)
        self.s, self.t = (v.float().contiguous() for v in self.out_affine)

    def contract(self, pts, rep, rows, knn):
        """The fused launch: pts [B,N,3], rep [B,P,3], rows [B*N, C2] (the dense's raw GEMM output), knn [B, K*D, P] -> D [B*P, C*dm]."""
        B, N, _ = pts.shape
        P = rep.shape[1]
        K, Cm, C, dm = self.K, self.C_mid, self.C_mid + self.C2, self.dm
        out = torch.empty((B * P, C * dm), dtype=torch.float32, device=pts.device)
        if any(t.data_ptr() % 16 for t in (self.Wb, self.W0, self.W1, self.W2, out)):
            raise ValueError("FrozenPointCNN: the X-conv kernel moves Wb, W0, W1, W2 and its output in 16-byte pieces: unaligned operand")
        flops = 2 * B * P * (K * (3 * Cm + Cm * Cm) + 3 * K * K * K + 2 * K ** 4 + K * K * C + K * C * dm)
        _lib.call("pcl_xconv_level_infer_f32", _p(pts), _p(rep), _p(rows), _p(self.fs), _p(self.ft), _p(knn), B, N, P, self.K, self.D,
                  self.C_mid, self.C2, self.dm, _p(self.Wa), _p(self.sa), _p(self.ta), _p(self.Wb), _p(self.sb), _p(self.tb), _p(self.W0),
                  _p(self.W1), _p(self.sc1), _p(self.sh1), _p(self.W2), _p(self.b2), _p(self.wd), _p(self.bias), _p(out), out.shape[1],
                  _stream(), algo_bytes=4 * B * P * (C * dm + K * (4 + self.C2)), algo_flops=flops, tag=f"xconv{K}x{C}x{dm}")
        return out

    def run(self, pts, rep, x):
        """pts [B,N,3], rep [B,P,3], x [B*N, C_in] (plain rows, or the raw output of the stage below) -> raw [B*P, C_out]."""
        knn = knn_indices(rep.transpose(1, 2).contiguous(), pts.transpose(1, 2).contiguous(), self.K * self.D)
        if self.folded:
            rows = _rows_gemm(x, self.Wd, self.bd, self.ones, self.zeros, 0.0, tag="pt")
        else:
            rows = _rows_gemm(x, self.Wd, self.bd, tag="pt")
        return self.pointwise(self.contract(pts, rep, rows, knn))

    def pointwise(self, D):
        return _rows_gemm(D, self.Wp)


class FrozenPointCNN(_Frozen):
    """Frozen evaluator of ``networks.cls.pointcnn.PointCNNcls``: ``fnet(x [B,N,3], normal=None) -> [B, n_classes]``, the signature
    of ``net.forward``; ``fnet.run(x, normal=None)`` also returns the features of the four X-conv stages (channel-last ``[B, P,
    C]``).  Constructed directly; fp32 only (``precision`` other than ``"fp32"`` raises).  DESIGN.md section 29.

    ``fnet.levels`` names the plan per stage.  ``"fused"`` for a stage whose shape has a kernel (``pcl_xconv_level_infer_supported``;
    csrc/infer_xconv.hip): FPS where the module samples (the same operator), ``pcl_knn_f32`` -- whose ``[B, K*D, P]`` lists the
    kernel reads as they are, dilation included --, the per-point ``dense`` as one stats-free GEMM (its BatchNorm + ReLU ride in
    the kernel's gather), ONE ``pcl_xconv_level_infer_f32`` launch (local coordinates, the lift, the X-transform, ``X [lift |
    gathered rows]`` and the depthwise taps of every region, with everything in LDS; ``D [B*P, C*dm]`` is the only large tensor a
    stage writes) and the pointwise GEMM.  ``"module"`` otherwise -- an eval-mode copy of the stage's own module runs.

    Folds, all in fp64 at ``refresh()`` and rounded once: ``x_trans_0``'s BatchNorm (it follows the ReLU) into ``x_trans_1``; a
    stage's trailing BatchNorm (``SepConv`` activates, then normalises: the output is ``s * relu(raw) + t``) into the two linear
    maps that read it, the next stage's ``dense`` and the head's first layer, which consume ``raw`` with the ReLU in their operand
    load.  ``run()`` forms the returned features explicitly.  The head is three stats-free GEMMs and the mean over the points
    (Dropout is the identity).  ``refresh()`` re-reads weights and running statistics; ``net`` itself is never modified
    (parameters, buffers, ``training`` flags), and a stale evaluator keeps its constants until ``refresh()``."""

    NET = PointCNNcls

    def __init__(self, net, precision="fp32"):
        if precision != "fp32":
            raise ValueError(f"FrozenPointCNN: fp32 only, got precision={precision!r}")
        super().__init__(net, precision)

    @torch.no_grad()
    def refresh(self):
        net = self.net
        self.stages = [net.pcnn1] + list(net.pcnn2)
        self.plans, affine = [], None
        for i, stage in enumerate(self.stages):
            if _xconv_fusable(stage):
                plan = _FusedXConv(stage, affine)
                self.plans.append(("fused", plan))
                affine = plan.out_affine
            else:
                self.plans.append(("module", self._copy(i, stage)))
                affine = None
        self.levels = [k for k, _ in self.plans]
        fcn = list(net.fcn)
        self.head_fused = (len(fcn) == 3 and all(isinstance(m, Dense_Conv1d) for m in fcn) and _relu_mlp(fcn[0].mlp, 1)
                           and _relu_mlp(fcn[1].mlp, 1) and _relu_mlp(fcn[2].mlp, 1, bn=False, act=False))
        if self.head_fused:
            f32 = lambda t: t.detach().float().contiguous().clone()
            m1, m2, m3 = (m.mlp for m in fcn)
            W1, b1 = m1.weights[0], m1.biases[0]
            self.head_folded = affine is not None
            if self.head_folded:
                W1, b1 = fold_affine_into_linear(W1, b1, *affine)
                self.h_ones, self.h_zeros = torch.ones(W1.shape[1], device=W1.device), torch.zeros(W1.shape[1], device=W1.device)
            self.hW = [f32(W1), f32(m2.weights[0]), f32(m3.weights[0])]
            self.hb = [f32(b1), f32(m2.biases[0]), f32(m3.biases[0])]
            self.hc = [_eval_consts(m1, 0, fold_bias=False), _eval_consts(m2, 0, fold_bias=False)]
        else:
            self.head = self._copy("head", net.fcn)
        return self

    def __call__(self, x, normal=None):
        return self._forward(x, normal, False)[1]

    def run(self, x, normal=None):
        """-> ([features of the four stages: [B, P, C]], logits [B, n_classes])."""
        return self._forward(x, normal, True)

    @torch.no_grad()
    def _forward(self, x, normal, want_feats):
        """``want_feats``: also form every fused stage's features ``s * relu(raw) + t`` (a forward itself never needs them: what
        reads a fused stage reads ``raw``)."""
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[2] != 3:
            raise ValueError(f"FrozenPointCNN: x must be [B,N,3], got {tuple(getattr(x, 'shape', ()))}")
        self._require_f32_gpu(x)
        if normal is not None:
            self._require_f32_gpu(normal, "normal")
        B = x.shape[0]
        pts = x.contiguous()
        cur, affine = (pts if normal is None else normal.contiguous()), None      # cur [B, N, C]: plain rows, or raw with (s, t)
        feats = []
        for stage, (kind, plan) in zip(self.stages, self.plans):
            N = pts.shape[1]
            if kind == "fused":
                rep = stage.sampler(pts) if 0 < plan.P < N else pts
                cur = plan.run(pts, rep, cur.reshape(B * N, -1)).view(B, rep.shape[1], -1)
                affine = (plan.s, plan.t)
                if want_feats:
                    feats.append(torch.relu(cur) * plan.s + plan.t)
            else:
                fts = cur if affine is None else torch.relu(cur) * affine[0] + affine[1]
                rep, cur = plan((pts, fts))
                affine = None
                feats.append(cur)
            pts = rep.contiguous()
        P = pts.shape[1]
        if not self.head_fused:
            return feats, self.head(cur if affine is None else torch.relu(cur) * affine[0] + affine[1]).mean(dim=1)
        rows = cur.reshape(B * P, -1)
        if self.head_folded:
            y = _rows_gemm(rows, self.hW[0], self.hb[0], self.h_ones, self.h_zeros, 0.0)
        else:
            y = _rows_gemm(rows.contiguous(), self.hW[0], self.hb[0])
        y = _rows_gemm(y, self.hW[1], self.hb[1], *self.hc[0], 0.0)
        y = _rows_gemm(y, self.hW[2], self.hb[2], *self.hc[1], 0.0)
        return feats, y.view(B, P, -1).mean(dim=1)


# ---------------------------------------------------------------------------------------------- PointCNN part segmentation
def fold_taps(wd, bias_d, Wp):
    """The depthwise taps of a ``SepConv`` folded into its pointwise conv, in fp64: in evaluation mode the two are linear maps with
    nothing between them, so ``raw[o] = sum_{c,j} Wp[o, c*dm+j] (bias_d[c*dm+j] + sum_k wd[c,j,k] FX[k,c]) = bf[o] + sum_{k,c}
    Wf[o, k*C+c] FX[k,c]`` with ``Wf[o, k*C+c] = sum_j Wp[o, c*dm+j] wd[c,j,k]`` and ``bf = Wp bias_d``.  wd [C, dm, K], bias_d
    [C*dm], Wp [C_out, C*dm] -> (Wf [C_out, K*C], bf [C_out]).  The contraction shrinks from C*dm to K*C columns per region: worth
    it where dm > K (``encoder_0`` of PointCNN_partseg: dm = 86, K = 8)."""
    wd, bias_d, Wp = wd.detach().double(), bias_d.detach().double(), Wp.detach().double()
    C, dm, K = wd.shape
    Wf = torch.einsum("ocj,cjk->okc", Wp.reshape(Wp.shape[0], C, dm), wd).reshape(Wp.shape[0], K * C)
    return Wf.contiguous(), Wp @ bias_d


def fold_conv_fuse(fuse, affines):
    """``conv_fuse`` of a ``RandPointCNN_Decoder`` reads ``cat(stage output, skip)``; where both are ``s * relu(raw) + t`` their
    affines (``affines``: [(s, t), (s, t)] in fp64, the stage's first) fold into the two column blocks of its weight
    (``fold_affine_into_linear`` on the concatenated scale and shift) -> (W', b') in fp64, to be applied to ``relu(cat(raw,
    raw_skip))``."""
    mlp = fuse.mlp
    return fold_affine_into_linear(mlp.weights[0], mlp.biases[0], torch.cat([a[0] for a in affines]), torch.cat([a[1] for a in affines]))


def _xconv_seg_form(stage):
    """The plan of a stage of PointCNN_partseg (``RandPointCNN`` or ``RandPointCNN_Decoder``): ``"fx"`` -- the FX form of the level
    kernel and the taps folded into the pointwise weight -- where dm > K and that shape has a kernel; else ``"taps"`` where the tap
    form has one; else ``None`` (the stage's own module runs), as for a stage whose parts are not the stock ones."""
    if not isinstance(stage, (RandPointCNN, RandPointCNN_Decoder)) or not _xconv_stock_parts(stage.pointcnn):
        return None
    if isinstance(stage, RandPointCNN_Decoder) and not (isinstance(stage.conv_fuse, Dense_Conv1d) and _relu_mlp(stage.conv_fuse.mlp, 1)
                                                        and stage.conv_fuse.mlp.biases is not None):
        return None
    pc, xc = stage.pointcnn, stage.pointcnn.x_conv
    K, Cm, C2, dm = int(pc.K), int(xc.C_mid), int(xc.C_in), int(xc.end_conv.dm)
    if dm > K and _lib.size_query("pcl_xconv_level_infer_fx_supported", K, Cm, C2):
        return "fx"
    return "taps" if _lib.size_query("pcl_xconv_level_infer_supported", K, Cm, C2, dm) else None


class _FusedXConvSeg(_FusedXConv):
    """``_FusedXConv`` for the stages of PointCNN_partseg.  ``form == "fx"``: ``pcl_xconv_level_infer_fx_f32`` writes FX [B*P, K*C]
    and one GEMM with ``fold_taps``' (Wf, bf) gives ``raw`` (the taps and the pointwise weight themselves are not kept).
    ``"taps"``: the tap form with the row stride of D padded to a multiple of 4 (decoder_3: 37 columns in 40; the pointwise
    weight gets zero columns, D's pad columns are zeros)."""

    def __init__(self, stage, in_affine, form):
        super().__init__(stage, in_affine)
        self.form = form
        C = self.C_mid + self.C2
        if form == "fx":
            ec = stage.pointcnn.x_conv.end_conv
            Wf, bf = fold_taps(ec.depthwise, ec.depthwise_bias, ec.pointwise.weights[0])
            self.Wf, self.bf = Wf.float().contiguous(), bf.float().contiguous()
            self.wd = self.bias = self.Wp = None
            self.ldo = self.K * C
        else:
            self.ldo = -(-C * self.dm // 4) * 4
            if self.ldo != C * self.dm:
                Wp = torch.zeros((self.Wp.shape[0], self.ldo), dtype=torch.float32, device=self.Wp.device)
                Wp[:, :C * self.dm] = self.Wp
                self.Wp = Wp

    def contract(self, pts, rep, rows, knn):
        """The fused launch -> FX [B*P, K*C] (``"fx"``) or D [B*P, ldo] (``"taps"``)."""
        B, N, _ = pts.shape
        P = rep.shape[1]
        K, Cm, C, dm = self.K, self.C_mid, self.C_mid + self.C2, self.dm
        fx = self.form == "fx"
        cols = K * C if fx else C * dm
        out = (torch.empty if self.ldo == cols else torch.zeros)((B * P, self.ldo), dtype=torch.float32, device=pts.device)
        if any(t.data_ptr() % 16 for t in (self.Wb, self.W0, self.W1, self.W2, out)):
            raise ValueError("FrozenPointCNNPartseg: the X-conv kernel moves Wb, W0, W1, W2 and its output in 16-byte pieces: unaligned operand")
        flops = 2 * B * P * (K * (3 * Cm + Cm * Cm) + 3 * K * K * K + 2 * K ** 4 + K * K * C + (0 if fx else K * C * dm))
        head = (_p(pts), _p(rep), _p(rows), _p(self.fs), _p(self.ft), _p(knn), B, N, P, K, self.D, Cm, self.C2)
        consts = (_p(self.Wa), _p(self.sa), _p(self.ta), _p(self.Wb), _p(self.sb), _p(self.tb), _p(self.W0), _p(self.W1), _p(self.sc1),
                  _p(self.sh1), _p(self.W2), _p(self.b2))
        prof = dict(algo_bytes=4 * B * P * (cols + K * (4 + self.C2)), algo_flops=flops)
        if fx:
            _lib.call("pcl_xconv_level_infer_fx_f32", *head, *consts, _p(out), self.ldo, _stream(), tag=f"xconvfx{K}x{C}", **prof)
        else:
            _lib.call("pcl_xconv_level_infer_f32", *head, dm, *consts, _p(self.wd), _p(self.bias), _p(out), self.ldo, _stream(),
                      tag=f"xconv{K}x{C}x{dm}", **prof)
        return out

    def pointwise(self, D):
        """What ``run`` (pts [B,N,3], rep [B,P,3] -- a decoder's: the finer level's points, P > N allowed --, x [B*N, C_in]) puts
        behind the launch -> raw [B*P, C_out]."""
        return _rows_gemm(D, self.Wf, self.bf) if self.form == "fx" else _rows_gemm(D, self.Wp)


class _FuseConv:
    """Snapshot of a decoder's ``conv_fuse`` (Linear + bias, BatchNorm, ReLU on ``cat(stage output, skip)``).  ``affines``: the
    (s, t) of the two inputs in fp64, or None for an input that arrives as plain features.  With both, ``fold_conv_fuse`` folds
    them into the weight and ``run`` takes the two ``raw`` tensors (ReLU in the GEMM's operand load); otherwise the weight is the
    module's own and ``run`` takes features."""

    def __init__(self, fuse, affines):
        mlp = fuse.mlp
        self.folded = all(a is not None for a in affines)
        W, b = fold_conv_fuse(fuse, affines) if self.folded else (mlp.weights[0], mlp.biases[0])
        self.W, self.b = (t.detach().float().contiguous().clone() for t in (W, b))
        if self.folded:
            self.ones, self.zeros = torch.ones(self.W.shape[1], device=self.W.device), torch.zeros(self.W.shape[1], device=self.W.device)
        self.sc, self.sh = _eval_consts(mlp, 0, fold_bias=False)

    def run(self, a, skip):
        """a [R, C_out], skip [R, C_last] -> relu(bn(.)) [R, C_out], a stored feature."""
        X = torch.cat((a, skip), dim=1)
        Y = _rows_gemm(X, self.W, self.b, self.ones, self.zeros, 0.0) if self.folded else _rows_gemm(X, self.W, self.b)
        out = torch.empty_like(Y)
        _lib.call("pcl_bn_act_f32", _p(Y), _p(self.sc), _p(self.sh), 0.0, Y.shape[0], Y.shape[1], _p(out), _stream())
        return out


def _plain(d, affine):
    """Features from what a stage hands on: ``d`` itself, or ``s * relu(raw) + t`` for a fused stage's ``raw``."""
    return d if affine is None else torch.relu(d) * affine[0] + affine[1]


class FrozenPointCNNPartseg(_Frozen):
    """Frozen evaluator of ``networks.seg.pointcnn_partseg.PointCNN_partseg``: ``fnet(x [B,N,3], normal=None) -> [B, part_num, N]``,
    the signature of ``net.forward`` (``normal`` is ignored there too); ``fnet.run(x)`` also returns the features of the eight
    stages, channel-last (four encoders, then the four decoders' fused outputs).  Constructed directly; fp32 only.  DESIGN.md
    section 30.

    ``fnet.levels``: ``"fused"`` or ``"module"`` per stage, encoder_0 .. encoder_3, decoder_0 .. decoder_3 (``_xconv_seg_form``).
    A fused stage is FPS where the module samples, ``pcl_knn_f32``, the per-point ``dense`` as one stats-free GEMM, ONE launch of
    the level kernel and one GEMM.  encoder_0 (dm = 86 > K = 8) takes the FX form: the kernel writes ``FX [B*N, K*C = 1536]`` and
    the GEMM contracts it with ``fold_taps``' weight -- the ``[B, N, 16512]`` tensor of the module and its 16512 -> 256 pointwise
    conv do not exist.  The other fused stages (encoder_1, decoder_2, decoder_3) take the tap form.  A decoder's representatives
    are the finer level's points, its points the coarser level's; no sampling.  Its ``conv_fuse`` is one stats-free GEMM on
    ``cat(raw, raw_skip)`` with both trailing affines folded into the weight where both producers are fused (``_FuseConv``), then
    BatchNorm + ReLU: a stored feature.  ``"module"``: an eval-mode copy of the stage's own module (the four K = 16 stages, whose
    tiles do not fit the kernel's LDS plan, and any stage with a part that is not the stock one).

    All folds are made in fp64 at ``refresh()`` and rounded once.  ``net`` itself is never modified (parameters, buffers,
    ``training`` flags); a stale evaluator keeps its constants until ``refresh()``."""

    NET = PointCNN_partseg

    def __init__(self, net, precision="fp32"):
        if precision != "fp32":
            raise ValueError(f"FrozenPointCNNPartseg: fp32 only, got precision={precision!r}")
        super().__init__(net, precision)

    @torch.no_grad()
    def refresh(self):
        net = self.net
        self.stages = [net.encoder_0, net.encoder_1, net.encoder_2, net.encoder_3, net.decoder_0, net.decoder_1, net.decoder_2, net.decoder_3]
        self.plans, self.fuses, enc = [], [], []
        affine = None                                                  # of what the next stage's dense reads
        for i, stage in enumerate(self.stages):
            form = _xconv_seg_form(stage)
            skip = enc[7 - i] if i >= 4 else None                      # decoder_0 .. 3 fuse with encoder_3 .. 0; decoder_0 reads encoder_3
            if form is None:
                self.plans.append(("module", self._copy(i, stage)))
                out = None
            else:
                plan = _FusedXConvSeg(stage, affine, form)
                self.plans.append(("fused", plan))
                out = plan.out_affine
            if i < 4:
                enc.append(out)
                affine = out
            else:
                self.fuses.append(None if form is None else _FuseConv(stage.conv_fuse, [out, skip]))
                affine = None                                          # a decoder hands on relu(bn(.)): plain rows
        self.levels = [k for k, _ in self.plans]
        return self

    def __call__(self, x, normal=None):
        return self._forward(x, False)[1]

    def run(self, x, normal=None):
        """-> ([features of the eight stages: [B, P, C]], logits [B, part_num, N])."""
        return self._forward(x, True)

    @torch.no_grad()
    def _forward(self, x, want_feats):
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[2] != 3:
            raise ValueError(f"FrozenPointCNNPartseg: x must be [B,N,3], got {tuple(getattr(x, 'shape', ()))}")
        self._require_f32_gpu(x)
        B = x.shape[0]
        pts = x.contiguous()
        cur, feats, enc = (pts, pts, None), [], []                     # (points [B,P,3], data [B,P,C], its affine or None)
        for stage, (kind, plan) in zip(self.stages[:4], self.plans[:4]):
            p, d, aff = cur
            n = p.shape[1]
            if kind == "fused":
                rep = (stage.sampler(p) if 0 < plan.P < n else p).contiguous()
                cur = (rep, plan.run(p, rep, d.reshape(B * n, -1)).view(B, rep.shape[1], -1), (plan.s, plan.t))
            else:
                rep, f = plan((p, _plain(d, aff)))
                cur = (rep.contiguous(), f, None)
            enc.append(cur)
            if want_feats:
                feats.append(_plain(cur[1], cur[2]))
        low = enc[3]
        for j, (kind, plan) in enumerate(self.plans[4:]):
            (pl, dl, al), (ph, dh, ah) = low, enc[3 - j]
            nh = ph.shape[1]
            if kind == "fused":
                fuse = self.fuses[j]
                raw = plan.run(pl, ph, dl.reshape(B * pl.shape[1], -1))
                if fuse.folded:
                    f = fuse.run(raw, dh.reshape(B * nh, -1))
                else:
                    f = fuse.run(_plain(raw, (plan.s, plan.t)), _plain(dh, ah).reshape(B * nh, -1))
                f = f.view(B, nh, -1)
            else:
                _, f = plan((pl, _plain(dl, al)), (ph, _plain(dh, ah)))
            low = (ph, f, None)
            feats.append(f)
        return (feats if want_feats else []), low[1].permute(0, 2, 1)
