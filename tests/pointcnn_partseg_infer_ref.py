"""Evaluation-mode restatement of PointCNN part segmentation (misc/pointcnn.py, networks/seg/pointcnn_partseg.py) in plain torch,
fp64 by default, built on tests/pointcnn_infer_ref.py: the FX form of ``level`` (one X-conv stage up to ``X . [lift | gathered
rows]``, no taps), a decoder stage with its ``conv_fuse``, the whole network on given representatives and k-NN lists.  Nothing is
folded: the depthwise taps and the pointwise conv are applied one after the other, every BatchNorm where the module applies it.
Not a test file."""
import torch

import pointcnn_infer_ref as R
from pointconv_infer_ref import _sparse_weight, granule

# the stages of PointCNN_partseg (part_num = 50) with a kernel: K, D, C_mid, C2, dm.  decoder_2 has encoder_1's shape.
SHAPES = {"encoder_0": (8, 1, 64, 128, 86), "encoder_1": (12, 1, 64, 128, 1), "decoder_3": (8, 1, 12, 25, 1)}
FX_SHAPES = ("encoder_0",)                       # dm > K: the FX form and the folded taps
ENCODERS = ("encoder_0", "encoder_1", "encoder_2", "encoder_3")
DECODERS = ("decoder_0", "decoder_1", "decoder_2", "decoder_3")


def level_fx(c, pts, rep, rows, idx, dtype=torch.float64, audit=None):
    """``pointcnn_infer_ref.level`` without the taps: pts [B,N,3], rep [B,P,3], rows [B,N,C2], idx [B,P,K] -> FX [B, P, K*C] with
    column k*C + c."""
    B, P, K = idx.shape
    bidx = torch.arange(B, device=idx.device).view(B, 1, 1)
    il = idx.long()
    pts, rep, rows = pts.to(dtype), rep.to(dtype), rows.to(dtype)
    d = pts[bidx, il] - rep.unsqueeze(2)
    h = R.dense_layer(R.dense_layer(d, c["lift"][0], audit), c["lift"][1], audit)
    x = R.conv_layer(d.reshape(B, P, 3 * K), c["x0"], audit)
    x = R.dense_layer(x, c["x1"], audit)
    X = R.dense_layer(x, c["x2"], audit, act=False).reshape(B, P, K, K)
    _, _, fs, ft = c["dense"]
    f = (fs.to(dtype) * rows[bidx, il] + ft.to(dtype)).clamp(min=0)
    F = torch.cat([h, f], dim=-1)
    if audit is not None:
        audit.append(float(torch.matmul(X.abs().double(), F.abs().double()).max()) / (granule(X) * granule(F)))
    return torch.matmul(X, F).reshape(B, P, -1)


def decoder_consts(dec):
    """``stage_consts`` of a ``RandPointCNN_Decoder`` plus its ``conv_fuse`` layer."""
    c = R.stage_consts(dec)
    c["fuse"] = R.mlp_layer(dec.conv_fuse.mlp, 0)
    return c


def decoder_stage(c, pts_l, fts_l, pts_h, fts_h, idx):
    """A whole ``RandPointCNN_Decoder`` in fp64: the X-conv from the coarse level (pts_l, fts_l) onto the fine level's points pts_h
    with the lists idx [B, P_h, K] into pts_l, concat with fts_h, ``conv_fuse`` -> (raw of the X-conv, fused features)."""
    raw, f = R.stage(c, pts_l, pts_h, fts_l, idx)
    return raw, R.dense_layer(torch.cat((f, fts_h.double()), dim=2), c["fuse"])


def network(net, x, reps, knns):
    """fp64 evaluation of ``PointCNN_partseg`` on ``reps`` (the four encoders' representatives [B,P,3]) and ``knns`` (the eight
    stages' [B, K*D, P] lists) -> ([features of the eight stages, channel-last], [raw of the eight X-convs], logits [B, parts, N])."""
    lv, feats, raws = [], [], []
    pts, fts = x.double(), x.double()
    for name, rep, knn in zip(ENCODERS, reps, knns[:4]):
        c = R.stage_consts(getattr(net, name))
        raw, fts = R.stage(c, pts, rep.double(), fts, R.dilated(knn, c["D"]))
        pts = rep.double()
        lv.append((pts, fts))
        feats.append(fts)
        raws.append(raw)
    low = lv[3]
    for j, (name, knn) in enumerate(zip(DECODERS, knns[4:])):
        c = decoder_consts(getattr(net, name))
        ph, fh = lv[3 - j]
        raw, f = decoder_stage(c, low[0], low[1], ph, fh, R.dilated(knn, c["D"]))
        low = (ph, f)
        feats.append(f)
        raws.append(raw)
    return feats, raws, low[1].permute(0, 2, 1)


# ------------------------------------------------------------------------------------------------- the C entries
def level_call(dev, k, pts, rep, rows, knn, D, fx=False, guard=8):
    """``pcl_xconv_level_infer_f32`` (or, ``fx``, ``pcl_xconv_level_infer_fx_f32``) through the C ABI on the constants ``k``
    (``pointcnn_infer_ref.kernel_consts`` / ``plan_consts``): -> [B, P, C*dm] (``fx``: [B, P, K*C]) on the device.  The row stride is
    the column count rounded up to a multiple of 4 plus ``guard`` columns (decoder_3: 37 columns in 40 + 8); everything behind a
    row's columns must stay as it was."""
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.misc.ops import _p, _stream
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    k = {n: f32(t) for n, t in k.items() if t is not None}
    pts, rep, rows = f32(pts), f32(rep), f32(rows)
    knn = knn.to(device=dev, dtype=torch.int32).contiguous()
    B, N, _ = pts.shape
    P, C2 = rep.shape[1], rows.shape[2]
    C_mid = k["Wa"].shape[0]
    C = C_mid + C2
    K = int(round(k["W2"].shape[0] ** 0.5))
    dm = 0 if fx else k["wd"].shape[1]
    cols = K * C if fx else C * dm
    assert knn.shape == (B, K * D, P) and k["W0"].shape == (K * K, -(-3 * K // 16) * 16)
    ldo = -(-cols // 4) * 4 + guard
    out = torch.full((B * P, ldo), 7.0, device=dev)
    assert all(t.data_ptr() % 16 == 0 for t in (k["Wb"], k["W0"], k["W1"], k["W2"], out))
    head = (_p(pts), _p(rep), _p(rows), _p(k["fs"]), _p(k["ft"]), _p(knn), B, N, P, K, D, C_mid, C2)
    consts = tuple(_p(k[n]) for n in ("Wa", "sa", "ta", "Wb", "sb", "tb", "W0", "W1", "sc1", "sh1", "W2", "b2"))
    if fx:
        _lib.call("pcl_xconv_level_infer_fx_f32", *head, *consts, _p(out), ldo, _stream())
    else:
        _lib.call("pcl_xconv_level_infer_f32", *head, dm, *consts, _p(k["wd"]), _p(k["bias"]), _p(out), ldo, _stream())
    torch.cuda.synchronize()
    assert bool((out[:, cols:] == 7.0).all()), "wrote beyond its columns"
    return out[:, :cols].reshape(B, P, cols)


# ------------------------------------------------------------------------------------------------- exactly representable data
def exact_case(name, B, N, P, seed, wp_nnz=32):
    """``pointcnn_infer_ref.exact_case`` for the shape ``name`` of ``SHAPES`` (the same grids: coordinates on 1/8, raw rows on 1/2,
    weights in {-1, -1/2, 1/2, 1} with two nonzeros per row, the taps too).  An FX shape also gets a pointwise weight ``Wp``
    [C_out, C*dm] from the same set with ``wp_nnz`` nonzeros per row: every ``Wf[o, k*C+c] = sum_j Wp[o, c*dm+j] wd[c,j,k]`` is then a
    short sum of multiples of 1/4 -- exact in fp64 and an fp32 number -- and so is ``bf``."""
    K, D, CM, C2, dm = SHAPES[name]
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
    if name in FX_SHAPES:
        c["Wp"] = _sparse_weight(4 * CM, C * dm, half, g, nnz=wp_nnz)              # C_out = 4 C_mid
    data = {"pts": torch.randint(0, 9, (B, N, 3), generator=g).double() / 8, "rep": torch.randint(0, 9, (B, P, 3), generator=g).double() / 8,
            "rows": torch.randint(-2, 3, (B, N, C2), generator=g).double() / 2, "knn": R.knn_lists(B, K * D, P, N, g)}
    return c, data
