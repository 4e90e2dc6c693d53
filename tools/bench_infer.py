"""Evaluation forward of the PointNet++ classifiers: ``net.eval()`` + ``torch.no_grad()`` (the existing path) against
``frozen(net)`` (pointcloudlib_amd/inference.py).  SSG and MSG, B in {32, 256}, N = 1024, synthetic clouds; the two forms
alternate window by window in one process, device events around each window, median over the windows; peak
``torch.cuda.max_memory_allocated`` above the resident set of one forward of each form.  Prints one JSON line.

The part-seg PointNet++ nets (``--nets partseg_ssg partseg_msg``; B in {16, 64}, N = 2048 unless --batch / --points say otherwise)
compare three forms: ``eval`` (the network's default accumulation, fp64 flush every 32 terms), ``eval_acc0`` (a copy with
``set_accumulation(copy, 0)``: plain fp32 chains) and ``frozen``.

    python tools/bench_infer.py [--windows 7] [--iters 5] [--warmup 3] [--batch 32 256] [--nets ssg msg] [--points 1024]
                                [--precision fp32 bf16]

``--precision fp32 bf16`` adds ``frozen(net, precision="bf16")`` as one more form of every row (``frozen_bf16_*``; in the same
interleaved windows, the same estimator), its ratio to the fp32 frozen form, the top-1 agreement of the two over the batch, and
writes the JSON line to profiles/infer_bf16_bench_line.json as well.

``--nets pointnet`` compares ``net.eval()`` under ``no_grad`` with ``FrozenPointNet(net)`` (B in {8, 32, 256}, N = 1024; both forms
read the same dense [B,3,N] tensor) and writes the JSON line to profiles/infer_pointnet_bench_line.json; with ``--ragged`` the four
forms below, the frozen form reading the [B,N,3] clouds through a transposed view (profiles/infer_pointnet_ragged_bench_line.json).
With ``--precision fp32 bf16`` every row also carries ``FrozenPointNet(net, precision="bf16")`` (the ``frozen_bf16_*`` columns
above, same windows) and, recorded only, the max-abs distance of the global feature and the logits from an fp64 restatement under
both precisions (``*_err_fp64_*``); the line goes to profiles/infer_pointnet_bf16_bench_line.json instead.

``--nets pointnet_partseg`` compares ``net.eval()`` under ``no_grad`` with ``FrozenPointNetPartseg(net)`` (B in {16, 64}, N = 2048;
both forms read the same dense [B,3,N] tensor and the same one-hot label) with the peak memory of both, and writes the JSON line
to profiles/infer_pointnet_partseg_bench_line.json; with ``--ragged`` the four forms below
(profiles/infer_pointnet_partseg_ragged_bench_line.json).  With ``--precision fp32 bf16`` every row also carries
``FrozenPointNetPartseg(net, precision="bf16")`` (``frozen_bf16_ms``, ``bf16_vs_fp32``, ``bf16_below_fp32_min``, the max-abs logit
distance and the per-point top-1 agreement of the two precisions); the line goes to
profiles/infer_pointnet_partseg_bf16_bench_line.json instead.

``--nets pointconv`` compares ``net.eval()`` under ``no_grad`` with ``FrozenPointConv(net)`` (B in {32, 256}, N = 1024; both forms read the
same dense [B,3,N] tensor and the SAME ``net.precompute_sampling`` handle, so the index-producing kernels are in neither), with the
peak memory of both and, per fused level, the time of the ``pcl_pointconv_level_infer_f32`` call between two device events
(``level_kernel_ms``, with its flops: TF/s against the fp32 MFMA peak); the line goes to profiles/infer_pointconv_bench_line.json.
With ``--precision fp32 bf16`` every row also carries ``FrozenPointConv(net, precision="bf16")`` in the same windows
(``frozen_bf16_ms`` with its window minimum, ``bf16_vs_fp32``, ``bf16_below_fp32_min``, the max-abs logit distance and the top-1
agreement of the two precisions, recorded and not asserted) and ``level_kernel_ms_bf16``, the same per-level times of the
``pcl_pointconv_level_infer_bf16_f32`` calls; the line goes to profiles/infer_pointconv_bf16_bench_line.json instead.
``--frozen_only --precision bf16`` runs the bf16 form alone (for a kernel trace) and writes no file.

``--nets pointconv_partseg`` compares ``net.eval()`` under ``no_grad`` with ``FrozenPointConvPartseg(net)`` (B in {16, 64}, N = 2048;
both forms read the same [B,N,3] tensor and the SAME ``net.precompute_sampling`` handle), with the peak memory of both, the
per-call times of the ``pcl_pointconv_seg_level_infer_f32`` launches (``level_kernel_ms``) and, between device events around each
level of a frozen forward (``frozen_level_ms``: sa0..sa3, in0..in3, head; ``in3_contract`` and ``in3_linear`` inside in3), the
shares of the two ``"module"`` levels and of the launches that write and read in3's ``[B N, 2048]`` contraction output; the line
goes to profiles/infer_pointconv_partseg_bench_line.json.  With ``--precision fp32 bf16`` every row also carries
``FrozenPointConvPartseg(net, precision="bf16")`` in the same interleaved windows, on the same tensor and the same sampling handle
(``frozen_bf16_ms`` with its window minimum and maximum, ``bf16_vs_fp32``, ``bf16_below_fp32_min``, the max-abs logit distance and the
per-point top-1 agreement of the two precisions, recorded and not asserted), ``level_kernel_ms_bf16`` (the per-call times of the
``pcl_pointconv_seg_level_infer_bf16_f32`` launches) and ``frozen_level_ms_bf16`` with the shares of the two ``"module"`` levels and
of in3's Linear in the bf16 forward; the line goes to profiles/infer_pointconv_partseg_bf16_bench_line.json instead.
``--frozen_only --precision bf16`` runs the bf16 form alone (for a kernel trace) and writes no file.
``--nets pointconv_partseg --wide`` adds ``FrozenPointConvPartseg(net, wide_levels=True)`` as one more interleaved form on the same
tensor and the same sampling handle (``frozen_wide_ms`` with its window minimum and maximum and its peak memory,
``wide_below_frozen_min``: the wide form's median against the default frozen form's window minimum, the max-abs logit distance of
the two), ``level_kernel_ms_wide`` (the per-call times and TF/s of the two ``pcl_pointconv_wide_level_infer_f32`` launches) and
``frozen_level_ms_wide`` (device events around each level and the head, and inside sa3, in0 and in3 around the launch with its ``Uf``
GEMM and around the level's Linear -- ``sa3_linear`` and ``in0_linear`` are the 8192 -> 512 Linears on B 36 and B 64 rows), with the
share of sa3 + in0 and of their two Linears; with ``--precision fp32 bf16`` the same for the bf16 forms (``frozen_bf16_wide_ms``,
``wide_below_frozen_min_bf16``, ``frozen_level_ms_bf16_wide``).  The line goes to
profiles/infer_pointconv_partseg_wide_bench_line.json.

``--nets pointcnn`` compares ``net.eval()`` under ``no_grad`` with ``FrozenPointCNN(net)`` (B in {32, 256}, N = 1024; both forms read
the same [B,N,3] tensor and run their own FPS and k-NN), with the peak memory of both, ``frozen_below_eval_min`` (the frozen median
against ``net.eval()``'s window minimum) and, per stage, the time of the ``pcl_xconv_level_infer_f32`` call between two device events
(``level_kernel_ms``, with its flops; ``level_kernel_share``: their sum over the frozen median); the line goes to
profiles/infer_pointcnn_bench_line.json.  fp32 only.

``--nets pointcnn_partseg`` compares ``net.eval()`` under ``no_grad`` with ``FrozenPointCNNPartseg(net)`` (B in {16, 64}, N = 2048; both
forms read the same [B,N,3] tensor and run their own FPS and k-NN), with the peak memory of both, ``frozen_below_eval_min``, the
plans (``levels``), the time of every ``pcl_xconv_level_infer_fx_f32`` / ``pcl_xconv_level_infer_f32`` call between two device events
(``level_kernel_ms``) and device events around every stage and every fused ``conv_fuse`` (``frozen_stage_ms``; ``module_stages_share``:
the stages that run as their own module over the sum); the line goes to profiles/infer_pointcnn_partseg_bench_line.json.  fp32 only.

``--ragged`` measures batches of clouds with different point counts instead (``frozen(net)(..., lengths=...)``): per net and batch,
lengths drawn once with a fixed seed uniformly from [N/2, N] (the largest forced to N), and four forms in interleaved windows --
(a) ``dense`` frozen at N, (b) ``ragged_full`` with every length = N, (c) ``ragged`` with the drawn lengths, (d) ``loop``: B calls
with B = 1, each on a cloud's own points.  The JSON line also goes to profiles/infer_ragged_bench_line.json.
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _window(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def _peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def _pointnet_fp64(net, x_cf, chunk=16):
    """fp64 restatement of ``PointNet`` in evaluation mode: x_cf [B,3,N] -> (global feature [B,1024], logits)."""
    mlp = net.convs
    feats = []
    for b0 in range(0, x_cf.shape[0], chunk):
        z = x_cf[b0:b0 + chunk].transpose(1, 2).double()
        for l in range(mlp.n_layers):
            rm, rv = getattr(mlp, f"running_mean_{l}").double(), getattr(mlp, f"running_var_{l}").double()
            scale = mlp.gammas[l].double() * torch.rsqrt(rv + mlp.eps)
            y = z @ mlp.weights[l].double().t()
            if mlp.biases is not None:
                y = y + mlp.biases[l].double()
            y = scale * (y - rm) + mlp.betas[l].double()
            z = torch.where(y > 0, y, y * mlp.slope)
        feats.append(z.max(dim=1)[0])
    feat = torch.cat(feats)
    def linear(m, t):
        t = t @ m.weight.double().t()
        return t if m.bias is None else t + m.bias.double()

    bn = net.bn6
    h = (linear(net.linear1, feat) - bn.running_mean.double()) * torch.rsqrt(bn.running_var.double() + bn.eps) * bn.weight.double() \
        + bn.bias.double()
    return feat, linear(net.linear2, h.clamp(min=0.0))


def _pointconv_level_times(fwd, entry="pcl_pointconv_level_infer_f32", repeats=5):
    """Per fused level of a FrozenPointConv forward: the ``entry`` call between two device events (average of ``repeats`` forwards;
    the events' own dispatch gaps are inside), its flops and the TF/s they give."""
    from pointcloudlib_amd import _lib
    timer = _lib.KernelTimer(names=[entry])
    _lib.PROFILER = timer
    try:
        for _ in range(repeats):
            fwd()
        torch.cuda.synchronize()
    finally:
        _lib.PROFILER = None
    out = {}
    for (_, tag), r in timer.summary().items():
        out[tag] = {"ms": round(r["avg_ms"], 4), "gflop": round(r["algo_flops"] / 1e9, 2),
                    "tflops": round(r["algo_flops"] / (r["avg_ms"] * 1e-3) / 1e12, 1)}
    return out


def _pointcnn_partseg_stage_times(fnet, fwd, repeats=5):
    """Device events around every stage of FrozenPointCNNPartseg forwards (a fused stage: k-NN, dense GEMM, the launch and the GEMM
    behind it; a module stage: the whole module, a decoder's ``conv_fuse`` included) and around every fused ``conv_fuse``
    (``<stage>_fuse``): average ms over ``repeats`` (the events' dispatch gaps are inside)."""
    marks = []
    names = ["encoder_0", "encoder_1", "encoder_2", "encoder_3", "decoder_0", "decoder_1", "decoder_2", "decoder_3"]

    def timed(fn, key):
        def wrapper(*args, **kw):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn(*args, **kw)
            b.record()
            marks.append((key, a, b))
            return out
        return wrapper

    plans, saved = list(fnet.plans), []
    for i, (kind, plan) in enumerate(plans):
        if kind == "fused":
            saved.append((plan, "run"))
            plan.run = timed(plan.run, names[i])
            if i >= 4:
                saved.append((fnet.fuses[i - 4], "run"))
                fnet.fuses[i - 4].run = timed(fnet.fuses[i - 4].run, names[i] + "_fuse")
        else:
            fnet.plans[i] = (kind, timed(plan, names[i]))
    try:
        for _ in range(repeats):
            fwd()
        torch.cuda.synchronize()
    finally:
        fnet.plans[:] = plans
        for obj, attr in saved:
            delattr(obj, attr)
    out = {}
    for key, a, b in marks:
        out[key] = out.get(key, 0.0) + a.elapsed_time(b) / repeats
    return {k: round(v, 4) for k, v in out.items()}


def _partseg_level_times(fpcs, fwd, repeats=5, split=(7,)):
    """Device events around every level, the head, and the two halves of the fused levels ``split`` (by default in3's: the launch
    that writes the contraction output, the Linear that reads it; keys ``<level>_contract``, ``<level>_linear``) of
    FrozenPointConvPartseg forwards: average ms over ``repeats`` (the events' dispatch gaps are inside)."""
    marks = []

    def timed(fn, key):
        def wrapper(*args, **kw):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn(*args, **kw)
            b.record()
            marks.append((key(*args), a, b))
            return out
        return wrapper

    names = list(fpcs.net.LEVELS)
    saved = [(fpcs, "_level", fpcs._level), (fpcs, "_head", fpcs._head)]
    fpcs._level, fpcs._head = timed(fpcs._level, lambda i, *r: names[i]), timed(fpcs._head, lambda *r: "head")
    for i in split:
        if fpcs.levels[i] == "fused":
            plan = fpcs.plans[i][1]
            saved += [(plan, "contract", plan.contract), (plan.linear, "run", plan.linear.run)]
            plan.contract = timed(plan.contract, lambda *r, n=names[i]: f"{n}_contract")
            plan.linear.run = timed(plan.linear.run, lambda *r, n=names[i]: f"{n}_linear")
    try:
        for _ in range(repeats):
            fwd()
        torch.cuda.synchronize()
    finally:
        for obj, attr, fn in saved:
            if attr in obj.__dict__:
                delattr(obj, attr)
    out = {}
    for key, a, b in marks:
        out[key] = out.get(key, 0.0) + a.elapsed_time(b) / repeats
    return {k: round(v, 4) for k, v in out.items()}


def _ragged_case(kind, fnet, xyz, nrm, extra, a, fnet_bf16=None):
    """The four forms of --ragged for one net and batch (same window estimator as the dense rows)."""
    import numpy as np
    B, N, _ = xyz.shape
    dev = xyz.device
    lengths = np.random.default_rng(12345).integers(N // 2, N + 1, B)
    lengths[int(lengths.argmax())] = N
    full = torch.full((B,), N, dtype=torch.int32, device=dev)
    drawn = torch.from_numpy(lengths.astype(np.int32)).to(dev)
    own = [(xyz[b:b + 1, :n].contiguous(), nrm[b:b + 1, :n].contiguous(), *(e[b:b + 1] for e in extra)) for b, n in enumerate(lengths.tolist())]

    def loop():
        return [fnet(*args) for args in own]

    forms = [("dense", lambda: fnet(xyz, nrm, *extra)), ("ragged_full", lambda: fnet(xyz, nrm, *extra, lengths=full)),
             ("ragged", lambda: fnet(xyz, nrm, *extra, lengths=drawn)), ("loop", loop)]
    if fnet_bf16 is not None:
        forms += [("dense_bf16", lambda: fnet_bf16(xyz, nrm, *extra)), ("ragged_bf16", lambda: fnet_bf16(xyz, nrm, *extra, lengths=drawn))]
    for _ in range(a.warmup):
        for _, fn in forms:
            fn()
    times = {name: [] for name, _ in forms}
    for w in range(a.windows):
        for name, fn in (forms if w % 2 == 0 else forms[::-1]):
            times[name].append(_window(fn, a.iters))
    case = {"net": kind, "B": B, "N": N, "mean_length": round(float(lengths.mean()), 1), "min_length": int(lengths.min())}
    for name, fn in forms:
        case[f"{name}_ms"] = round(statistics.median(times[name]), 4)
        case[f"{name}_ms_min"] = round(min(times[name]), 4)
        case[f"{name}_ms_max"] = round(max(times[name]), 4)
        if name != "loop":
            case[f"{name}_peak_mib"] = round(_peak(fn) / 2**20, 2)
    case["ragged_full_vs_dense"] = round(case["ragged_full_ms"] / case["dense_ms"], 4)
    case["ragged_vs_dense"] = round(case["ragged_ms"] / case["dense_ms"], 4)
    case["loop_vs_ragged"] = round(case["loop_ms"] / case["ragged_ms"], 2)
    if fnet_bf16 is not None:
        case["dense_bf16_vs_fp32"] = round(case["dense_bf16_ms"] / case["dense_ms"], 4)
        case["ragged_bf16_vs_fp32"] = round(case["ragged_bf16_ms"] / case["ragged_ms"], 4)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, nargs="+", default=None, help="default: 32 256 (cls), 16 64 (part-seg, pointnet_partseg), 8 32 256 (pointnet)")
    ap.add_argument("--nets", nargs="+", default=["ssg", "msg"], choices=["ssg", "msg", "partseg_ssg", "partseg_msg", "pointnet", "pointnet_partseg", "pointconv",
                                                                                "pointconv_partseg", "pointcnn", "pointcnn_partseg"])
    ap.add_argument("--points", type=int, default=None, help="default: 1024 (cls), 2048 (part-seg)")
    ap.add_argument("--frozen_only", action="store_true", help="run only the frozen form (for a kernel trace)")
    ap.add_argument("--precision", nargs="+", default=["fp32"], choices=["fp32", "bf16"],
                    help="fp32 bf16: frozen(net, precision='bf16') as one more form of every row")
    ap.add_argument("--wide", action="store_true", help="pointconv_partseg: FrozenPointConvPartseg(net, wide_levels=True) as one more form")
    ap.add_argument("--ragged", action="store_true", help="ragged batches: dense / ragged at full length / ragged / per-cloud loop")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_infer.py needs a GPU")
    from pointcloudlib_amd import synth
    from pointcloudlib_amd.inference import frozen
    from pointcloudlib_amd.networks.cls.pointnet2 import PointNet2_cls, PointNetMSG
    dev = torch.device("cuda")
    cls_only = all(k in ("ssg", "msg", "pointnet", "pointconv", "pointcnn") for k in a.nets)
    pointcnn_only = all(k == "pointcnn" for k in a.nets)
    pcnn_partseg_only = all(k == "pointcnn_partseg" for k in a.nets)
    if ("pointcnn" in a.nets or "pointcnn_partseg" in a.nets) and (a.ragged or "bf16" in a.precision):
        raise SystemExit("bench_infer.py: FrozenPointCNN and FrozenPointCNNPartseg are fp32 only and have no ragged form")
    pointnet_only = all(k == "pointnet" for k in a.nets)
    pn_partseg_only = all(k == "pointnet_partseg" for k in a.nets)
    pointconv_only = all(k == "pointconv" for k in a.nets)
    pc_partseg_only = all(k == "pointconv_partseg" for k in a.nets)
    if a.wide and (not pc_partseg_only or a.ragged or a.frozen_only):
        raise SystemExit("bench_infer.py: --wide goes with --nets pointconv_partseg alone, without --ragged or --frozen_only")
    if a.ragged and ("pointconv" in a.nets or "pointconv_partseg" in a.nets):
        raise SystemExit("bench_infer.py: PointConv's sampling has no ragged form")
    res = {"N": (a.points or 1024) if cls_only else (a.points or 2048), "windows": a.windows, "iters": a.iters, "cases": []}
    if a.ragged:
        del res["N"]                 # every --ragged case carries its own N (classifiers and part-seg nets share one line)
    for kind in a.nets:
        seg = kind.startswith("partseg")
        pn_seg = kind == "pointnet_partseg"
        pc_seg = kind == "pointconv_partseg"
        pcnn_seg = kind == "pointcnn_partseg"
        N = a.points or (2048 if seg or pn_seg or pc_seg or pcnn_seg else 1024)
        torch.manual_seed(0)
        if seg:
            from pointcloudlib_amd.misc.layers import set_accumulation
            from pointcloudlib_amd.networks.seg.pointnet2_partseg import PointNet2_partseg, PointNetMSG as PartsegMSG
            net = (PointNet2_partseg if kind == "partseg_ssg" else PartsegMSG)().to(dev).eval()
            net0 = set_accumulation(copy.deepcopy(net), 0)
        elif kind == "pointnet":
            from pointcloudlib_amd.inference import FrozenPointNet
            from pointcloudlib_amd.networks.cls.pointnet import PointNet
            net = PointNet().to(dev).eval()
        elif kind == "pointconv":
            from pointcloudlib_amd.inference import FrozenPointConv
            from pointcloudlib_amd.networks.cls.pointconv import PointConvDensityClsSsg
            net = PointConvDensityClsSsg().to(dev).eval()
        elif kind == "pointcnn":
            from pointcloudlib_amd.inference import FrozenPointCNN
            from pointcloudlib_amd.networks.cls.pointcnn import PointCNNcls
            net = PointCNNcls().to(dev).eval()
        elif pcnn_seg:
            from pointcloudlib_amd.inference import FrozenPointCNNPartseg
            from pointcloudlib_amd.networks.seg.pointcnn_partseg import PointCNN_partseg
            net = PointCNN_partseg().to(dev).eval()
        elif pn_seg:
            from pointcloudlib_amd.inference import FrozenPointNetPartseg
            from pointcloudlib_amd.networks.seg.pointnet_partseg import PointNet_partseg
            net = PointNet_partseg().to(dev).eval()
        elif pc_seg:
            from pointcloudlib_amd.inference import FrozenPointConvPartseg
            from pointcloudlib_amd.networks.seg.pointconv_partseg import PointConvDensity_partseg
            net = PointConvDensity_partseg().to(dev).eval()
        else:
            net = (PointNet2_cls if kind == "ssg" else PointNetMSG)().to(dev).eval()
        if kind == "pointnet":
            fpn = FrozenPointNet(net)

            def fnet(xyz, nrm, lengths=None):                 # the tool's call shape; [B,N,3] read through a transposed view
                return fpn(xyz.transpose(1, 2), lengths)
            fnet_bf16 = None
            if "bf16" in a.precision:
                fpn16 = FrozenPointNet(net, precision="bf16")

                def fnet_bf16(xyz, nrm, lengths=None):
                    return fpn16(xyz.transpose(1, 2), lengths)
        elif kind == "pointconv":
            fpc = FrozenPointConv(net)
            fnet_bf16 = fpc16 = FrozenPointConv(net, precision="bf16") if "bf16" in a.precision else None
        elif kind == "pointcnn":
            fcnn = FrozenPointCNN(net)
            fnet_bf16 = None
        elif pcnn_seg:
            fcnn = FrozenPointCNNPartseg(net)
            fnet_bf16 = None
        elif pc_seg:
            fpcs = FrozenPointConvPartseg(net)
            fnet_bf16 = fpcs16 = FrozenPointConvPartseg(net, precision="bf16") if "bf16" in a.precision else None
            fpcs_w = FrozenPointConvPartseg(net, wide_levels=True) if a.wide else None
            fpcs16_w = FrozenPointConvPartseg(net, precision="bf16", wide_levels=True) if a.wide and "bf16" in a.precision else None
        elif pn_seg:
            fps = FrozenPointNetPartseg(net)

            def fnet(xyz, nrm, onehot, lengths=None):         # the tool's call shape; [B,N,3] read through a transposed view
                return fps(xyz.transpose(1, 2), onehot, lengths)
            fnet_bf16 = None
            if "bf16" in a.precision:
                fps16 = FrozenPointNetPartseg(net, precision="bf16")

                def fnet_bf16(xyz, nrm, onehot, lengths=None):
                    return fps16(xyz.transpose(1, 2), onehot, lengths)
        else:
            fnet = frozen(net)
            fnet_bf16 = frozen(net, precision="bf16") if "bf16" in a.precision else None
        for B in a.batch or ([16, 64] if seg or pn_seg or pc_seg or pcnn_seg else [8, 32, 256] if kind == "pointnet" else [32, 256]):
            xyz = torch.from_numpy(synth.gauss_ball(B, N, 1)).to(dev)
            nrm = torch.from_numpy(synth.unit_normals(B, N, 2)).to(dev)
            extra = ()
            if seg or pn_seg:
                onehot = torch.zeros(B, 16, device=dev)
                onehot[torch.arange(B), torch.arange(B) % 16] = 1.0
                extra = (onehot,)

            def eval_fwd(net=net):
                with torch.no_grad():
                    return net(xyz, nrm, *extra)

            def frozen_fwd():
                return fnet(xyz, nrm, *extra)

            def frozen_bf16_fwd():
                return fnet_bf16(xyz, nrm, *extra)

            if kind == "pointnet":
                x_cf = xyz.transpose(1, 2).contiguous()       # the network's input layout, made once: both forms read it

                def eval_fwd(net=net):
                    with torch.no_grad():
                        return net(x_cf)

                def frozen_fwd():
                    return fpn(x_cf)

                def frozen_bf16_fwd():
                    return fpn16(x_cf)

            if kind == "pointconv":
                x_cf = xyz.transpose(1, 2).contiguous()       # the network's input layout, made once: both forms read it
                samp = net.precompute_sampling(x_cf)          # ... and one sampling handle

                def eval_fwd(net=net):
                    with torch.no_grad():
                        return net(x_cf, sampling=samp)

                def frozen_fwd():
                    return fpc(x_cf, sampling=samp)

                def frozen_bf16_fwd():
                    return fpc16(x_cf, sampling=samp)

            if kind == "pointcnn" or pcnn_seg:
                def eval_fwd(net=net):
                    with torch.no_grad():
                        return net(xyz)

                def frozen_fwd():
                    return fcnn(xyz)

            if pc_seg:
                samp = net.precompute_sampling(xyz)           # one sampling handle feeds both forms

                def eval_fwd(net=net):
                    with torch.no_grad():
                        return net(xyz, sampling=samp)

                def frozen_fwd():
                    return fpcs(xyz, sampling=samp)

                def frozen_bf16_fwd():
                    return fpcs16(xyz, sampling=samp)

            if pn_seg:
                x_cf = xyz.transpose(1, 2).contiguous()       # the network's input layout, made once: both forms read it

                def eval_fwd(net=net):
                    with torch.no_grad():
                        return net(x_cf, onehot)

                def frozen_fwd():
                    return fps(x_cf, onehot)

                def frozen_bf16_fwd():
                    return fps16(x_cf, onehot)

            if a.ragged:
                res["cases"].append(_ragged_case(kind, fnet, xyz, nrm, extra, a, fnet_bf16))
                continue
            if a.frozen_only:
                forms = [("frozen", frozen_fwd)] if "fp32" in a.precision or kind not in ("pointconv", "pointconv_partseg") else []
            elif seg:
                forms = [("eval", eval_fwd), ("eval_acc0", lambda: eval_fwd(net0)), ("frozen", frozen_fwd)]
            else:
                forms = [("eval", eval_fwd), ("frozen", frozen_fwd)]
            if fnet_bf16 is not None:
                forms.append(("frozen_bf16", frozen_bf16_fwd))
            wide_forms = []                                   # (suffix of the result keys, default form, wide form)
            if a.wide and "fp32" in a.precision:
                wide_forms.append(("", "frozen", fpcs_w))
            if a.wide and fpcs16_w is not None:
                wide_forms.append(("_bf16", "frozen_bf16", fpcs16_w))
            for _, base, form in wide_forms:
                forms.append((f"{base}_wide", lambda form=form: form(xyz, sampling=samp)))
            for _ in range(a.warmup):
                for _, fn in forms:
                    fn()
            times = {name: [] for name, _ in forms}
            for w in range(a.windows):
                for name, fn in (forms if w % 2 == 0 else forms[::-1]):
                    times[name].append(_window(fn, a.iters))
            case = {"net": kind, "B": B, "N": N} if seg or pn_seg or pc_seg or pcnn_seg else {"net": kind, "B": B}
            for name, fn in forms:
                case[f"{name}_ms"] = round(statistics.median(times[name]), 4)
                case[f"{name}_ms_min"] = round(min(times[name]), 4)
                if fnet_bf16 is not None or pc_seg:
                    case[f"{name}_ms_max"] = round(max(times[name]), 4)
                case[f"{name}_peak_mib"] = round(_peak(fn) / 2**20, 1)
            if not a.frozen_only:
                case["speedup"] = round(case["eval_ms"] / case["frozen_ms"], 3)
                if seg:
                    case["speedup_vs_acc0"] = round(case["eval_acc0_ms"] / case["frozen_ms"], 3)
                if pc_seg or pcnn_seg or kind == "pointcnn":
                    case["frozen_below_eval_min"] = case["frozen_ms"] < case["eval_ms_min"]
                if seg or pn_seg or pc_seg or pcnn_seg or kind in ("pointconv", "pointcnn"):
                    case["mem_ratio"] = round(case["eval_peak_mib"] / max(case["frozen_peak_mib"], 0.1), 1)
                with torch.no_grad():
                    case["max_abs_logit_diff"] = float((eval_fwd() - frozen_fwd()).abs().max())
            if fnet_bf16 is not None and "frozen" in times:
                case["bf16_vs_fp32"] = round(case["frozen_bf16_ms"] / case["frozen_ms"], 4)
                case["bf16_below_fp32_min"] = case["frozen_bf16_ms"] < case["frozen_ms_min"]
                lf, lb = frozen_fwd(), frozen_bf16_fwd()
                case["max_abs_logit_diff_bf16_fp32"] = float((lf - lb).abs().max())
                cdim = -1 if pc_seg else 1                    # FrozenPointConvPartseg's logits are [B, N, parts]: per-point top-1
                case["top1_agreement_bf16_fp32"] = float((lf.argmax(cdim) == lb.argmax(cdim)).float().mean())
                if kind == "pointnet" and not a.frozen_only:  # recorded, not asserted: distance from fp64 under both precisions
                    f64, l64 = _pointnet_fp64(net, x_cf)
                    for tag, form in (("fp32", fpn), ("bf16", fpn16)):
                        feat, logits = form.run(x_cf)
                        case[f"feature_err_fp64_{tag}"] = float((feat.double() - f64).abs().max())
                        case[f"logit_err_fp64_{tag}"] = float((logits.double() - l64).abs().max())
                    case["top1_agreement_bf16_fp64"] = float((lb.argmax(1) == l64.argmax(1)).float().mean())
            if kind == "pointconv" and "frozen" in times:
                case["level_kernel_ms"] = _pointconv_level_times(frozen_fwd)
            if kind == "pointconv" and fnet_bf16 is not None:
                case["level_kernel_ms_bf16"] = _pointconv_level_times(frozen_bf16_fwd, "pcl_pointconv_level_infer_bf16_f32")
            if kind == "pointcnn" and "frozen" in times:
                case["levels"] = fcnn.levels
                lk = case["level_kernel_ms"] = _pointconv_level_times(frozen_fwd, "pcl_xconv_level_infer_f32")
                case["level_kernel_share"] = round(sum(v["ms"] for v in lk.values()) / case["frozen_ms"], 4)
            if pcnn_seg and "frozen" in times:
                case["levels"] = fcnn.levels
                case["level_kernel_ms"] = {**_pointconv_level_times(frozen_fwd, "pcl_xconv_level_infer_fx_f32"),
                                           **_pointconv_level_times(frozen_fwd, "pcl_xconv_level_infer_f32")}
                st = case["frozen_stage_ms"] = _pointcnn_partseg_stage_times(fcnn, frozen_fwd)
                names = [n for n in st if not n.endswith("_fuse")]
                case["module_stages_share"] = round(sum(st[n] for n, k in zip(names, fcnn.levels) if k == "module") / sum(st.values()), 4)
            if pc_seg and "frozen" in times:
                case["levels"] = fpcs.levels
                case["level_kernel_ms"] = _pointconv_level_times(frozen_fwd, "pcl_pointconv_seg_level_infer_f32")
                lt = case["frozen_level_ms"] = _partseg_level_times(fpcs, frozen_fwd)
                total = sum(v for k, v in lt.items() if not k.startswith("in3_"))
                case["module_levels_share"] = round(sum(lt[n] for n, k in zip(net.LEVELS, fpcs.levels) if k == "module") / total, 4)
                if "in3_contract" in lt:
                    case["in3_contraction_output_share"] = round((lt["in3_contract"] + lt["in3_linear"]) / total, 4)
            if pc_seg and fnet_bf16 is not None:
                case["levels"] = fpcs16.levels
                case["level_kernel_ms_bf16"] = _pointconv_level_times(frozen_bf16_fwd, "pcl_pointconv_seg_level_infer_bf16_f32")
                lt = case["frozen_level_ms_bf16"] = _partseg_level_times(fpcs16, frozen_bf16_fwd)
                total = sum(v for k, v in lt.items() if not k.startswith("in3_"))
                case["module_levels_share_bf16"] = round(sum(lt[n] for n, k in zip(net.LEVELS, fpcs16.levels) if k == "module") / total, 4)
                if "in3_linear" in lt:
                    case["in3_linear_share_bf16"] = round(lt["in3_linear"] / total, 4)
            for sfx, base, form in wide_forms:
                fwd = dict(forms)[f"{base}_wide"]
                case[f"wide_below_frozen_min{sfx}"] = case[f"{base}_wide_ms"] < case[f"{base}_ms_min"]
                case[f"wide_vs_frozen{sfx}"] = round(case[f"{base}_wide_ms"] / case[f"{base}_ms"], 4)
                case[f"max_abs_logit_diff_wide{sfx}"] = float((dict(forms)[base]() - fwd()).abs().max())
                case[f"levels{sfx}_wide"] = form.levels
                case[f"level_kernel_ms{sfx}_wide"] = _pointconv_level_times(fwd, "pcl_pointconv_wide_level_infer_f32")
                lt = case[f"frozen_level_ms{sfx}_wide"] = _partseg_level_times(form, fwd, split=(3, 4, 7))
                total = sum(v for k, v in lt.items() if "_" not in k)
                case[f"wide_levels_share{sfx}"] = round((lt["sa3"] + lt["in0"]) / total, 4)
                case[f"wide_linears_share{sfx}"] = round((lt["sa3_linear"] + lt["in0_linear"]) / total, 4)
            res["cases"].append(case)
    print(json.dumps(res))
    if a.wide:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "infer_pointconv_partseg_wide_bench_line.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
    elif "bf16" in a.precision and not a.ragged and not ((pointnet_only or pn_partseg_only or pointconv_only or pc_partseg_only) and a.frozen_only):
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        name = ("infer_pointnet_bf16_bench_line.json" if pointnet_only else
                "infer_pointnet_partseg_bf16_bench_line.json" if pn_partseg_only else
                "infer_pointconv_bf16_bench_line.json" if pointconv_only else
                "infer_pointconv_partseg_bf16_bench_line.json" if pc_partseg_only else "infer_bf16_bench_line.json")
        with open(os.path.join(ROOT, "profiles", name), "w") as f:
            f.write(json.dumps(res) + "\n")
    elif pointnet_only and not a.frozen_only:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "infer_pointnet_ragged_bench_line.json" if a.ragged else "infer_pointnet_bench_line.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
    elif pointconv_only and not a.frozen_only:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "infer_pointconv_bench_line.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
    elif pc_partseg_only and not a.frozen_only:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "infer_pointconv_partseg_bench_line.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
    elif pointcnn_only and not a.frozen_only:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "infer_pointcnn_bench_line.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
    elif pcnn_partseg_only and not a.frozen_only:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "infer_pointcnn_partseg_bench_line.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
    elif pn_partseg_only and not a.frozen_only:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        name = "infer_pointnet_partseg_ragged_bench_line.json" if a.ragged else "infer_pointnet_partseg_bench_line.json"
        with open(os.path.join(ROOT, "profiles", name), "w") as f:
            f.write(json.dumps(res) + "\n")
    elif a.ragged:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "infer_ragged_bench_line.json"), "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
