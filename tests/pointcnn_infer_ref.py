"""Evaluation-mode restatement of PointCNN classification (misc/pointcnn.py, networks/cls/pointcnn.py) in plain torch, fp64 by
default: one X-conv stage up to the depthwise taps (``level``), a whole stage, the whole network.  Index lists and representatives
are arguments, so sampling and the neighbour search are not part of what is compared.  Every BatchNorm is applied where the module
applies it -- none is folded into a neighbouring Linear: ``Dense_*`` is Linear + bias, BatchNorm, ReLU; ``Conv`` (``x_trans_0``) and
``SepConv`` are Linear, ReLU, THEN BatchNorm.  A layer is ``(W [out, in], b | None, scale | None, shift | None)`` with (scale,
shift) the BatchNorm's affine map in evaluation mode.  Not a test file."""
import torch

from pointconv_infer_ref import _sparse_weight, granule

STAGES = {1: (8, 1, 12, 24, 16), 2: (12, 2, 24, 48, 2), 3: (16, 2, 48, 96, 2), 4: (16, 3, 96, 192, 2)}     # K, D, C_mid, C2, dm


def bn_affine(gamma, beta, rm, rv, eps):
    scale = gamma.detach().double() / torch.sqrt(rv.double() + eps)
    return scale, beta.detach().double() - scale * rm.double()


def mlp_layer(mlp, l):
    W = mlp.weights[l].detach().double()
    b = None if mlp.biases is None else mlp.biases[l].detach().double()
    if not mlp.bn:
        return W, b, None, None
    return (W, b) + bn_affine(mlp.gammas[l], mlp.betas[l], getattr(mlp, f"running_mean_{l}"), getattr(mlp, f"running_var_{l}"), mlp.eps)


def bn_last(bn):
    return bn_affine(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)


def stage_consts(stage):
    """The parameters and running statistics of a ``RandPointCNN`` as fp64 layers (nothing folded)."""
    pc, xc = stage.pointcnn, stage.pointcnn.x_conv
    ec = xc.end_conv
    return {"K": pc.K, "D": pc.D, "P": stage.P, "dense": mlp_layer(pc.dense.mlp, 0), "lift": [mlp_layer(xc.dense, 0), mlp_layer(xc.dense, 1)],
            "x0": (xc.x_trans_0.linear.weights[0].detach().double(), None) + bn_last(xc.x_trans_0.bn),
            "x1": mlp_layer(xc.x_trans_1.mlp, 0), "x2": mlp_layer(xc.x_trans_2.mlp, 0),
            "wd": ec.depthwise.detach().double(), "bias": ec.depthwise_bias.detach().double(),
            "Wp": ec.pointwise.weights[0].detach().double(), "out": bn_last(ec.bn)}


def _linear(x, W, b, audit, extra=None):
    """x W^T + b; ``audit``: (largest sum of |products| and |addends| of any output) / (the granule all of them share)."""
    if audit is not None:
        big = x.abs().double() @ W.abs().double().t()
        gran = granule(x) * granule(W)
        for t in (b, extra):
            if t is not None:
                big, gran = big + t.abs().double(), min(gran, granule(t))
        audit.append(float(big.max()) / gran)
    y = x @ W.to(x.dtype).t()
    return y if b is None else y + b.to(x.dtype)


def dense_layer(x, layer, audit=None, act=True):
    """``Dense_Conv1d/2d``: Linear + bias, BatchNorm, ReLU (misc/pointcnn.py: Dense_Conv1d)."""
    W, b, sc, sh = layer
    y = _linear(x, W, b, audit, sh)
    if sc is not None:
        y = sc.to(x.dtype) * y + sh.to(x.dtype)
    return y.clamp(min=0) if act else y


def conv_layer(x, layer, audit=None):
    """``Conv`` / the tail of ``SepConv``: Linear, ReLU, THEN BatchNorm (misc/pointcnn.py: Conv.forward, SepConv.forward_x)."""
    W, b, sc, sh = layer
    return sc.to(x.dtype) * _linear(x, W, b, audit, sh).clamp(min=0) + sh.to(x.dtype)


def level(c, pts, rep, rows, idx, dtype=torch.float64, audit=None):
    """One stage from the dense's raw GEMM output up to and including the depthwise taps (PointCNN.forward after ``dense``'s Linear,
    XConv.forward_local, ``_XConvCore``): pts [B,N,3], rep [B,P,3], rows [B,N,C2] = fts W_dense^T + b, idx [B,P,K] (the dilated lists)
    -> D [B, P, C*dm] with column c*dm + j."""
    B, P, K = idx.shape
    bidx = torch.arange(B, device=idx.device).view(B, 1, 1)
    il = idx.long()
    pts, rep, rows = pts.to(dtype), rep.to(dtype), rows.to(dtype)
    d = pts[bidx, il] - rep.unsqueeze(2)                                              # [B,P,K,3]
    h = dense_layer(dense_layer(d, c["lift"][0], audit), c["lift"][1], audit)           # [B,P,K,C_mid]
    x = conv_layer(d.reshape(B, P, 3 * K), c["x0"], audit)
    x = dense_layer(x, c["x1"], audit)
    X = dense_layer(x, c["x2"], audit, act=False).reshape(B, P, K, K)
    _, _, fs, ft = c["dense"]
    f = (fs.to(dtype) * rows[bidx, il] + ft.to(dtype)).clamp(min=0)                   # the dense's BatchNorm + ReLU, then the gather
    F = torch.cat([h, f], dim=-1)                                                      # [B,P,K,C]
    wd, bias = c["wd"].to(dtype), c["bias"].to(dtype)
    if audit is not None:
        audit.append(float(torch.matmul(X.abs().double(), F.abs().double()).max()) / (granule(X) * granule(F)))
    FX = torch.matmul(X, F)                                                            # [B,P,K,C]
    if audit is not None:
        big = torch.einsum("bpkc,cjk->bpcj", FX.abs().double(), wd.abs().double()).reshape(B, P, -1) + bias.abs().double()
        audit.append(float(big.max()) / min(granule(FX) * granule(wd), granule(bias)))
    C, dm = wd.shape[0], wd.shape[1]
    return torch.einsum("bpkc,cjk->bpcj", FX, wd).reshape(B, P, C * dm) + bias


def dilated(knn, D):
    """[B, K*D, P] as pcl_knn_f32 writes it -> the lists of PointCNN.region_indices, [B, P, K]."""
    return knn[:, 0::D, :].permute(0, 2, 1).contiguous()


def stage(c, pts, rep, fts, idx):
    """A whole ``RandPointCNN`` in fp64 on given representatives and lists -> (raw = the pointwise conv's output, features)."""
    W, b, _, _ = c["dense"]
    rows = fts.double() @ W.t() + b
    raw = level(c, pts, rep, rows, idx) @ c["Wp"].t()
    sc, sh = c["out"]
    return raw, sc * raw.clamp(min=0) + sh


def network(net, x, normal, reps, knns):
    """fp64 evaluation of ``PointCNNcls`` on ``reps`` (the four stages' representatives [B,P,3]) and ``knns`` (their [B, K*D, P]
    lists) -> ([features of the four stages, channel-last], logits)."""
    pts, fts, feats = x.double(), (x if normal is None else normal).double(), []
    for st, rep, knn in zip([net.pcnn1] + list(net.pcnn2), reps, knns):
        c = stage_consts(st)
        _, fts = stage(c, pts, rep.double(), fts, dilated(knn, c["D"]))
        feats.append(fts)
        pts = rep.double()
    y = fts
    for i, m in enumerate(net.fcn):
        y = dense_layer(y, mlp_layer(m.mlp, 0), act=i < 2)
    return feats, y.mean(dim=1)


# ------------------------------------------------------------------------------------------------- the constants of the C entry
def kernel_consts(c):
    """The layers of ``stage_consts`` / ``exact_case`` as ``pcl_xconv_level_infer_f32`` takes them, in fp64: Linear biases folded
    into the shifts, ``x_trans_0``'s BatchNorm into ``x_trans_1``, Wb and W0 zero-padded to multiples of 16."""
    def folded(layer):
        W, b, sc, sh = layer
        return W, sc, sh if b is None else sh + sc * b

    def pad16(W):
        r, q = (-(-n // 16) * 16 for n in W.shape)
        out = torch.zeros(r, q, dtype=W.dtype, device=W.device)
        out[:W.shape[0], :W.shape[1]] = W
        return out

    (Wa, sa, ta), (Wb, sb, tb) = folded(c["lift"][0]), folded(c["lift"][1])
    W0, _, s0, t0 = c["x0"]
    W1, sc1, sh1 = folded(c["x1"])
    W2, b2, _, _ = c["x2"]
    return {"fs": c["dense"][2], "ft": c["dense"][3], "Wa": Wa, "sa": sa, "ta": ta, "Wb": pad16(Wb), "sb": sb, "tb": tb, "W0": pad16(W0),
            "W1": W1 * s0.unsqueeze(0), "sc1": sc1, "sh1": sh1 + sc1 * (W1 @ t0), "W2": W2, "b2": b2, "wd": c["wd"], "bias": c["bias"]}


def plan_consts(plan):
    """The same dict from an evaluator's plan (``inference._FusedXConv``): what a forward hands the kernel."""
    return {k: getattr(plan, k) for k in ("fs", "ft", "Wa", "sa", "ta", "Wb", "sb", "tb", "W0", "W1", "sc1", "sh1", "W2", "b2", "wd", "bias")}


def level_call(dev, k, pts, rep, rows, knn, D):
    """``pcl_xconv_level_infer_f32`` through the C ABI on the constants ``k`` (``kernel_consts`` / ``plan_consts``; any dtype and
    device): pts [B,N,3], rep [B,P,3], rows [B,N,C2], knn [B, K*D, P] -> [B, P, C*dm] on the device.  Eight guard columns behind
    every output row must stay as they were."""
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.misc.ops import _p, _stream
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    k = {n: f32(t) for n, t in k.items()}
    pts, rep, rows = f32(pts), f32(rep), f32(rows)
    knn = knn.to(device=dev, dtype=torch.int32).contiguous()
    B, N, _ = pts.shape
    P, C2 = rep.shape[1], rows.shape[2]
    C, dm, K = k["wd"].shape
    C_mid = C - C2
    assert knn.shape == (B, K * D, P) and k["W0"].shape == (K * K, -(-3 * K // 16) * 16)
    ldo = C * dm + 8
    out = torch.full((B * P, ldo), 7.0, device=dev)
    assert all(t.data_ptr() % 16 == 0 for t in (k["Wb"], k["W0"], k["W1"], k["W2"], out))
    _lib.call("pcl_xconv_level_infer_f32", _p(pts), _p(rep), _p(rows), _p(k["fs"]), _p(k["ft"]), _p(knn), B, N, P, K, D, C_mid, C2, dm,
              _p(k["Wa"]), _p(k["sa"]), _p(k["ta"]), _p(k["Wb"]), _p(k["sb"]), _p(k["tb"]), _p(k["W0"]), _p(k["W1"]), _p(k["sc1"]),
              _p(k["sh1"]), _p(k["W2"]), _p(k["b2"]), _p(k["wd"]), _p(k["bias"]), _p(out), ldo, _stream())
    torch.cuda.synchronize()
    assert bool((out[:, C * dm:] == 7.0).all()), "wrote beyond its columns"
    return out[:, :C * dm].reshape(B, P, C * dm)


# ------------------------------------------------------------------------------------------------- cases of the level kernel
def knn_lists(B, KD, P, N, g):
    """Random lists [B, K*D, P] from [0, N), repeats allowed, with 0 and N - 1 forced into rows the dilation keeps."""
    knn = torch.randint(0, N, (B, KD, P), generator=g, dtype=torch.int32)
    knn[0, 0, 0], knn[-1, 0, -1] = 0, N - 1
    return knn


def exact_case(s, B, N, P, seed):
    """Exactly representable data for stage ``s`` of ``STAGES``: coordinates on a 1/8 grid, the dense's raw rows on a 1/2 grid,
    weights in {-1, -1/2, 1/2, 1} (``x_trans_2``: {-1, 1}) with two nonzeros per row -- the depthwise taps too --, BatchNorm scales
    1 (``x_trans_0``'s: powers of two from {1/2, 1, 2}, the fold stays exact), shifts and biases on a 1/8 grid.  Every product and
    partial sum of the stage is then an integer multiple of one power of two and (``level(..., audit=)`` measures it) below 2^24
    times it, so fp32 arithmetic in any order -- the folded order included -- gives the fp64 result.  -> (layers as
    ``stage_consts`` gives them, dict of CPU fp64 inputs with ``knn`` [B, K*D, P])."""
    K, D, CM, C2, dm = STAGES[s]
    g = torch.Generator().manual_seed(seed)
    half, unit = [-1.0, -0.5, 0.5, 1.0], [-1.0, 1.0]
    eighths = lambda n: torch.randint(-2, 5, (n,), generator=g).double() / 8
    ones = lambda n: torch.ones(n, dtype=torch.float64)
    pow2 = lambda n: torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n,), generator=g)]
    C = CM + C2
    wd = torch.stack([_sparse_weight(dm, K, half, g) for _ in range(C)])                  # [C, dm, K]
    c = {"K": K, "D": D, "P": P, "dense": (None, None, ones(C2), eighths(C2)),
         "lift": [(_sparse_weight(CM, 3, half, g), eighths(CM), ones(CM), eighths(CM)),
                  (_sparse_weight(CM, CM, half, g), None, ones(CM), eighths(CM))],
         "x0": (_sparse_weight(K * K, 3 * K, half, g), None, pow2(K * K), eighths(K * K)),
         "x1": (_sparse_weight(K * K, K * K, half, g), eighths(K * K), ones(K * K), eighths(K * K)),
         "x2": (_sparse_weight(K * K, K * K, unit, g), eighths(K * K), None, None),
         "wd": wd, "bias": eighths(C * dm)}
    data = {"pts": torch.randint(0, 9, (B, N, 3), generator=g).double() / 8, "rep": torch.randint(0, 9, (B, P, 3), generator=g).double() / 8,
            "rows": torch.randint(-2, 3, (B, N, C2), generator=g).double() / 2, "knn": knn_lists(B, K * D, P, N, g)}
    return c, data
