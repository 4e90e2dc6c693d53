"""Frozen inference with bf16 matrix operands on the GPU (``frozen(net, precision="bf16")``, pcl_sa_level_infer_bf16_f32).

Two yardsticks.  Where every value that the kernel rounds to bf16 is a small integer, nothing is lost and the launch must equal
the fp32 launch and the fp64 evaluation BIT FOR BIT: that pins every k, row and column mapping.  On random data the launch must
lie within the derived forward error bound of tests/bf16_bound.py, elementwise (tests/test_inference_bf16_cpu.py shows that the
bound is loose against rounding noise and tight against a mapping defect).  The fp64 restatement takes the constants the launch
is given (fp32 weights, scale, shift).  Geometry, shape table and helpers are those of tests/test_inference_gpu.py and
tests/test_inference_ragged_gpu.py.

The random and network cases print their worst error / bound ratio before they assert (``-s`` shows it); DESIGN.md section 17 is
where those figures are recorded."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# (ns, C1, C2, C3): every width triple with a kernel, ns as in the shape table's rows
_TRIPLES = [(16, 32, 32, 64), (64, 64, 64, 128), (128, 64, 96, 128), (64, 128, 128, 256)]


def _P(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launch(entry, Ws, scales, shifts, slope, xyz, new_xyz, feat, idx, cnt, inline, Uf=None):
    """One launch of ``entry`` (either precision) through the C ABI into a column slice of a wider, sentinel-filled buffer.
    Ws[0] fp32 [C1, 3 + C]; Ws[l >= 1] fp32 [C_l, C_{l-1}], handed over as bf16 to the bf16 entry."""
    from pointcloudlib_amd import _lib
    B, N, _ = xyz.shape
    m, ns = idx.shape[1], idx.shape[2]
    C = feat.shape[-1]
    W0 = Ws[0].contiguous()
    C1 = W0.shape[0]
    feat2 = feat.reshape(B * N, C).contiguous()
    if not inline and Uf is None:
        Uf = torch.empty(B * N, C1, device=xyz.device)
        Wf = W0[:, 3:].contiguous()
        _lib.call("pcl_linear_fwd_rows_f32", _P(feat2), _P(Wf), None, None, None, 0.0, B * N, C, C1, _P(Uf), None, None, None, _stream())
    L = len(Ws)
    dt = torch.bfloat16 if "bf16" in entry else torch.float32
    Wl = [None] + [w.to(dt).contiguous() for w in Ws[1:]]
    widths = (ctypes.c_int32 * L)(*[w.shape[0] for w in Ws])
    c_W = (ctypes.c_void_p * L)(*[_P(w) for w in Wl])
    c_sc = (ctypes.c_void_p * L)(*[_P(t) for t in scales])
    c_sh = (ctypes.c_void_p * L)(*[_P(t) for t in shifts])
    CL = Ws[-1].shape[0]
    ldo, col0 = CL + 8, 5
    out = torch.full((B * m, ldo), 7.0, device=xyz.device)
    _lib.call(entry, _P(xyz), _P(new_xyz), None if inline else _P(Uf), _P(W0), _P(feat2) if inline else None,
              _P(W0[:, 3:]) if inline else None, C if inline else 0, W0.shape[1], _P(idx), _P(cnt), B, N, m, ns, L, widths, c_W,
              c_sc, c_sh, float(slope), _P(out), ldo, col0, _stream())
    torch.cuda.synchronize()
    assert bool((out[:, :col0] == 7.0).all()) and bool((out[:, col0 + CL:] == 7.0).all()), "wrote outside its column slice"
    return out[:, col0:col0 + CL].reshape(B, m, CL)


BF16, FP32 = "pcl_sa_level_infer_bf16_f32", "pcl_sa_level_infer_f32"


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. exact, bit for bit
def _sparse_pm1(rows, cols, nnz, g):
    """[rows, cols] with ``nnz`` entries of +-1 per row at random columns (coinciding draws leave fewer), the rest 0."""
    W = torch.zeros(rows, cols)
    for _ in range(nnz):
        c = torch.randint(0, cols, (rows,), generator=g)
        W[torch.arange(rows), c] = torch.where(torch.rand(rows, generator=g) < 0.5, -1.0, 1.0)
    return W


@pytest.mark.parametrize("ns,c1,c2,c3", _TRIPLES)
@pytest.mark.parametrize("inline", [True, False])
def test_bf16_level_exact_case_bit_for_bit(dev, ns, c1, c2, c3, inline):
    from bf16_bound import act, grouped_rows
    from test_inference_gpu import _kernel_case
    C = 3 if inline else 128
    _, xyz, new_xyz, feat, idx, cnt, _ = _kernel_case(dev, ns, [C, c1, c2, c3], 0.0, seed=ns + c1 + c2)
    g = torch.Generator().manual_seed(c1 + c3 + int(inline))
    xyz = torch.randint(0, 8, xyz.shape, generator=g).float().to(dev)
    new_xyz = torch.randint(0, 8, new_xyz.shape, generator=g).float().to(dev)
    feat = torch.randint(-3, 4, feat.shape, generator=g).float().to(dev)
    Ws = [_sparse_pm1(c1, 3 + C, 2, g).to(dev), _sparse_pm1(c2, c1, 4, g).to(dev), _sparse_pm1(c3, c2, 4, g).to(dev)]
    scales = [torch.ones(c, device=dev) for c in (c1, c2, c3)]
    shifts = [torch.zeros(c, device=dev) for c in (c1, c2, c3)]
    # the fp64 evaluation, and the precondition on it: every activation that gets rounded to bf16 is an integer of magnitude
    # <= 256 (8 significant bits: exact in bf16), the last layer's far below 2^24 (exact in fp32, in any order)
    x, valid = grouped_rows(xyz, new_xyz, feat, idx, cnt)
    a = x
    for l, W in enumerate(Ws):
        a = act(a @ W.double().t(), 0.0)
        assert bool((a == a.round()).all()) and float(a.max()) > 0
        assert float(a.abs().max()) <= (256 if l < 2 else 4 * 256), f"layer {l + 1}: {float(a.abs().max())}"
    want = a.masked_fill(~valid.unsqueeze(-1), float("-inf")).max(dim=2)[0]
    assert float(want.max()) > 0 and len(want.unique()) > 4           # not a degenerate (all-zero) case
    Uf = None if inline else (feat.reshape(-1, C) @ Ws[0][:, 3:].t()).contiguous()     # integers: exact in any order
    got = _launch(BF16, Ws, scales, shifts, 0.0, xyz, new_xyz, feat, idx, cnt, inline, Uf)
    again = _launch(BF16, Ws, scales, shifts, 0.0, xyz, new_xyz, feat, idx, cnt, inline, Uf)
    f32 = _launch(FP32, Ws, scales, shifts, 0.0, xyz, new_xyz, feat, idx, cnt, inline, Uf)
    assert _same(got, again), "two calls differ"
    assert torch.equal(got.double(), want), f"bf16 launch differs from fp64: {int((got.double() != want).sum())} of {want.numel()} elements"
    assert _same(got, f32), "bf16 launch differs from the fp32 launch"


# ------------------------------------------------------------------------------------------------ 2. random, in the bound
def _random_case(dev, ns, spec, slope):
    from pointcloudlib_amd.inference import _eval_consts
    from test_inference_gpu import _kernel_case
    mlp, xyz, new_xyz, feat, idx, cnt, _ = _kernel_case(dev, ns, spec, slope, seed=ns + spec[1] + spec[2] + int(10 * slope))
    Ws = [w.detach() for w in mlp.weights]
    consts = [_eval_consts(mlp, l) for l in range(mlp.n_layers)]
    return Ws, [c[0] for c in consts], [c[1] for c in consts], xyz, new_xyz, feat, idx, cnt


def _shapes():
    from test_inference_gpu import _SHAPES
    return _SHAPES


@pytest.mark.parametrize("row", range(8))
@pytest.mark.parametrize("slope", [0.0, 0.2])
def test_bf16_level_random_case_within_the_bound(dev, row, slope):
    from bf16_bound import level_ref_and_bound, worst_ratio
    ns, spec, inline = _shapes()[row]
    Ws, sc, sh, xyz, new_xyz, feat, idx, cnt = _random_case(dev, ns, spec, slope)
    got = _launch(BF16, Ws, sc, sh, slope, xyz, new_xyz, feat, idx, cnt, inline)
    again = _launch(BF16, Ws, sc, sh, slope, xyz, new_xyz, feat, idx, cnt, inline)
    assert _same(got, again), "two calls differ"
    ref, bound = level_ref_and_bound(xyz, new_xyz, feat, idx, cnt, Ws, sc, sh, slope)
    ratio = worst_ratio(got, ref, bound)
    f32 = worst_ratio(_launch(FP32, Ws, sc, sh, slope, xyz, new_xyz, feat, idx, cnt, inline), ref, bound)
    print(f"BF16BOUND ns={ns} spec={spec} slope={slope}: worst |bf16 - fp64| / bound = {ratio:.4f} "
          f"(max abs {float((got.double() - ref).abs().max()):.3e}; the fp32 launch: {f32:.5f})")
    assert bool(torch.isfinite(got).all())
    assert ratio <= 1.0, f"bf16 launch is {ratio:.3f} x the bound away from fp64"


# ------------------------------------------------------------------------------------------------ 3. geometry independence
@pytest.mark.parametrize("row", [0, 1, 4])
def test_bf16_group_result_does_not_depend_on_the_launch(dev, row):
    """Cloud 1's groups in a launch of their own (B = 1: other group tiles, other workgroups) against their rows of the batch."""
    ns, spec, inline = _shapes()[row]
    Ws, sc, sh, xyz, new_xyz, feat, idx, cnt = _random_case(dev, ns, spec, 0.2)
    B, N, _ = xyz.shape
    Uf = None
    if not inline:                       # one table for both launches: the comparison is about the level kernel
        Uf = (feat.reshape(B * N, -1) @ Ws[0][:, 3:].t()).contiguous()
    batch = _launch(BF16, Ws, sc, sh, 0.2, xyz, new_xyz, feat, idx, cnt, inline, Uf)
    alone = _launch(BF16, Ws, sc, sh, 0.2, xyz[1:2].contiguous(), new_xyz[1:2].contiguous(), feat[1:2].contiguous(),
                    idx[1:2].contiguous(), cnt[1:2].contiguous(), inline, None if Uf is None else Uf[N:2 * N].contiguous())
    assert _same(batch[1:2], alone)


# ------------------------------------------------------------------------------------------------ 4. networks
def _network(task, kind, dev):
    from test_inference_ragged_gpu import _net
    return _net(task, kind, dev)          # BN statistics perturbed, explicit tie stride


def _check_levels(net, fnet, f32net, xyz, nrm, feats, samp):
    from bf16_bound import level_ref_and_bound, worst_ratio
    from pointcloudlib_amd.inference import _Fused
    cur_xyz, cur_feat = xyz, nrm
    n_fused = 0
    for i, (plans, plans32, (new_xyz, idxs)) in enumerate(zip(fnet.levels, f32net.levels, samp["levels"])):
        col = 0
        for j, ((kind, plan), (kind32, plan32), ic) in enumerate(zip(plans, plans32, idxs)):
            assert kind == kind32 and type(plan) is type(plan32), f"level {i} scale {j}: plan differs from fp32's"
            if kind != "fused":
                continue
            assert isinstance(plan, _Fused) and plan.precision == "bf16"
            cl = plan.widths[-1]
            Ws = [plan.W0] + plan.Ws[1:]
            ref, bound = level_ref_and_bound(cur_xyz, new_xyz, cur_feat, ic[0], ic[1], Ws, plan.scales, plan.shifts, plan.slope, plan.use_xyz)
            got = feats[i][:, :, col:col + cl]
            ratio = worst_ratio(got, ref, bound)
            print(f"BF16NET level {i} scale {j} widths {plan.widths}: worst error / bound = {ratio:.4f}")
            assert ratio <= 1.0, f"level {i} scale {j}: {ratio:.3f} x the bound away from fp64"
            col += cl
            n_fused += 1
        cur_xyz, cur_feat = new_xyz, feats[i]
    return n_fused


@pytest.mark.parametrize("kind", ["ssg", "msg"])
def test_bf16_classifier_levels_within_the_bound(dev, kind):
    from pointcloudlib_amd import synth
    from pointcloudlib_amd.inference import frozen
    net = _network("cls", kind, dev)
    B, N = 4, 1024
    xyz, nrm = torch.from_numpy(synth.gauss_ball(B, N, 0)).to(dev), torch.from_numpy(synth.unit_normals(B, N, 1)).to(dev)
    samp = net.precompute_sampling(xyz)
    fnet, f32net = frozen(net, precision="bf16"), frozen(net)
    feats, logits = fnet.run(xyz, nrm, sampling=samp)
    torch.cuda.synchronize()
    assert _check_levels(net, fnet, f32net, xyz, nrm, feats, samp) == (2 if kind == "ssg" else 6)
    assert logits.shape == (B, 40) and bool(torch.isfinite(logits).all())
    assert type(fnet.head) is type(f32net.head)


def test_bf16_partseg_levels_within_the_bound(dev):
    from pointcloudlib_amd import synth
    from pointcloudlib_amd.inference import frozen
    from test_inference_ragged_gpu import _onehot
    net = _network("seg", "ssg", dev)
    B, N = 2, 1024
    xyz, nrm = torch.from_numpy(synth.gauss_ball(B, N, 0)).to(dev), torch.from_numpy(synth.unit_normals(B, N, 1)).to(dev)
    samp = net.precompute_sampling(xyz)
    fnet, f32net = frozen(net, precision="bf16"), frozen(net)
    levels, logits = fnet.run(xyz, nrm, _onehot(dev, B), sampling=samp)
    torch.cuda.synchronize()
    assert _check_levels(net, fnet, f32net, xyz, nrm, levels[:3], samp) == 2
    assert logits.shape == (B, net.part_num, N) and bool(torch.isfinite(logits).all())
    assert [k for k, _ in fnet.fp.values()] == [k for k, _ in f32net.fp.values()] and fnet.head_fused == f32net.head_fused


# ------------------------------------------------------------------------------------------------ 5. ragged
_LENGTHS = [1024, 512, 513, 777]


def test_bf16_classifier_ragged_equals_every_cloud_alone(dev):
    from pointcloudlib_amd.inference import frozen
    from test_inference_ragged_gpu import _clouds
    net = _network("cls", "ssg", dev)
    fnet = frozen(net, precision="bf16")
    xyz, nrm = _clouds(dev, _LENGTHS, 1024, "nan")
    feats, logits = fnet.run(xyz, nrm, lengths=_LENGTHS)
    assert bool(torch.isfinite(logits).all())
    for b, n in enumerate(_LENGTHS):
        o_feats, o_logits = fnet.run(xyz[b:b + 1, :n].contiguous(), nrm[b:b + 1, :n].contiguous())
        for i, (f, o) in enumerate(zip(feats, o_feats)):
            assert _same(f[b:b + 1], o), f"cloud {b} (n={n}): level {i} feature differs from the cloud alone"
        assert _same(logits[b:b + 1], o_logits), f"cloud {b} (n={n}): logits differ from the cloud alone"


def test_bf16_partseg_ragged_equals_every_cloud_alone(dev):
    from pointcloudlib_amd.inference import frozen
    from test_inference_ragged_gpu import _clouds, _onehot
    net = _network("seg", "ssg", dev)
    fnet = frozen(net, precision="bf16")
    B, N = len(_LENGTHS), 1024
    onehot = _onehot(dev, B)
    xyz, nrm = _clouds(dev, _LENGTHS, N, "nan")
    levels, logits = fnet.run(xyz, nrm, onehot, lengths=_LENGTHS)
    for b, n in enumerate(_LENGTHS):
        o_levels, o_logits = fnet.run(xyz[b:b + 1, :n].contiguous(), nrm[b:b + 1, :n].contiguous(), onehot[b:b + 1])
        for name, f, o in zip(["sa1", "sa2", "sa3", "fp3", "fp2", "fp1"], levels, o_levels):
            rows = n if name == "fp1" else f.shape[1]
            assert _same(f[b:b + 1, :rows], o), f"cloud {b} (n={n}): {name} differs from the cloud alone"
        assert _same(logits[b:b + 1, :, :n], o_logits), f"cloud {b} (n={n}): logits differ from the cloud alone"
        assert bool(torch.isfinite(logits[b, :, :n]).all())
        assert not logits[b, :, n:].contiguous().view(torch.int32).any(), f"cloud {b}: logits of pad points"


# ------------------------------------------------------------------------------------------------ 6. contract
def test_bf16_frozen_contract(dev):
    from pointcloudlib_amd import synth
    from pointcloudlib_amd.inference import frozen
    net = _network("cls", "ssg", dev).train()
    B, N = 8, 1024
    xyz, nrm = torch.from_numpy(synth.gauss_ball(B, N, 3)).to(dev), torch.from_numpy(synth.unit_normals(B, N, 4)).to(dev)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    samp = net.precompute_sampling(xyz)
    f_default, f_fp32, f_bf16 = frozen(net), frozen(net, precision="fp32"), frozen(net, precision="bf16")
    d_feats, d_logits = f_default.run(xyz, nrm, sampling=samp)
    e_feats, e_logits = f_fp32.run(xyz, nrm, sampling=samp)
    assert _same(d_logits, e_logits) and all(_same(a, b) for a, b in zip(d_feats, e_feats)), 'precision="fp32" is not frozen(net)'
    out = f_bf16(xyz, nrm, sampling=samp)
    assert _same(out, f_bf16(xyz, nrm)), "a precomputed sampling handle changes the output"
    assert not _same(out, d_logits), "the bf16 path computed the fp32 result: is it the bf16 launch?"
    torch.cuda.synchronize()
    assert net.training and all(m.training for m in net.modules())
    after = net.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "frozen() modified the network"
    with torch.no_grad():                                    # the bf16 snapshot is stale until refresh()
        net.pointnet_modules[1].mlps[0].weights[1].mul_(1.25)
    stale = f_bf16(xyz, nrm, sampling=samp)
    fresh = f_bf16.refresh()(xyz, nrm, sampling=samp)
    torch.cuda.synchronize()
    assert _same(stale, out)
    assert not _same(fresh, out)
    assert _same(fresh, frozen(net, precision="bf16")(xyz, nrm, sampling=samp))


def test_bf16_frozen_forward_memory(dev):
    """The bound formula of test_frozen_forward_memory: the bf16 weights are construction-time constants, not forward allocations."""
    from pointcloudlib_amd import synth
    from pointcloudlib_amd.inference import frozen
    net = _network("cls", "ssg", dev)
    B, N = 32, 1024
    xyz, nrm = torch.from_numpy(synth.gauss_ball(B, N, 0)).to(dev), torch.from_numpy(synth.unit_normals(B, N, 1)).to(dev)
    samp = net.precompute_sampling(xyz)
    fnet = frozen(net, precision="bf16")
    fnet(xyz, nrm, sampling=samp)                 # warm-up: one-time allocations (constants, plans)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fnet(xyz, nrm, sampling=samp)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    level_out = B * 512 * 128 + B * 128 * 256 + B * 1024
    uf = B * 512 * 128                            # SA2's per-point table (SA1's normals fold inline)
    group_all = B * 128 * (3 + 256 + 256 + 512 + 1024)
    bound = 2 * 4 * (level_out + uf + group_all)
    assert out.shape == (B, 40)
    assert peak <= bound, f"bf16 frozen forward peak +{peak / 2**20:.1f} MiB > bound {bound / 2**20:.1f} MiB"
