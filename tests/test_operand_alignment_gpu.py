"""GPU: every alignment-dependent dispatch of csrc/ with operands that are NOT 16-byte aligned.

The tests elsewhere pass fresh allocations (256-byte aligned), so of every ``al16(...)`` predicate only the width half is ever false.
Here each op runs (a) aligned, (b) with one class of external operand at a time moved 4, 8 or 12 bytes behind a 16-byte boundary
(tests/misaligned.py) and (c) with all of them moved, through the public autograd entry points.  Nothing may raise.  Every run --
(a) included -- is compared with the same operation in fp64 PyTorch on the CPU under the bound the op's existing fp64 test uses
(named per test), and every shifted run with the aligned one: bit-equal where the inventory says the same kernels are selected
(SAME_KERNELS below: per family, the operand classes every kernel reads by scalars or the wrapper copies), else the largest difference is
printed and asserted under the same fp64 bound.

INVENTORY mirrors the table of DESIGN.md section 22: one row per function of csrc/*.hip that asks ``al16(...)``
(tests/test_operand_alignment_cpu.py fails when a function is missing here)."""
import contextlib
import copy

import pytest
import torch
from torch import nn

import oracle.torch_backend  # noqa: F401,E402  (registers the plain-PyTorch composite the tests compare against)

from misaligned import shift_module, shifted
from pointcloudlib_amd.misc.layers import PointwiseMLP

pytestmark = pytest.mark.gpu

_MLP, _GRP, _HEAD, _SEG, _PC, _XC, _KNN, _STEP = ("test_pointwise_mlp_plain_rows / test_pointwise_mlp_pooled", "test_forward_grouped",
                                                  "test_fc_head", "test_segment_pooling", "test_pointconv_contract", "test_xconv_core",
                                                  "test_knn_point_matmul_refuses_a_misaligned_cloud", "test_pointnet2_cls_whole_step")
_LIB = "none: every operand is carved by the library (256 bytes)"
_FROZEN = ("none among those the predicate asks about: inference.py folds the weights into tensors of its own (fresh allocations) and carves Uf "
           "and the workspaces; the callers' xyz / features are not its subject and go by scalars (strided reads)")
# (file, function) -> entry = the extern "C" entry points behind it; external = caller's operands the predicate covers;
# misaligned = what happens then (kernel | copy | error); case = the test
INVENTORY = {
    ("mlp.hip", "fwd_res_eligible"): dict(entry=["pcl_linear_fwd_rows_f32", "pcl_linear_fwd_f32", "pcl_mlp_stack_fwd_f32"],
                                          external="x (layer 0), W, bias -- asked for the opt-in bf16-plane form only; the fp32 kernel takes any 4-byte alignment (buffer loads)", misaligned="kernel: the staged forward (launch_linear_t)", case="test_resident_weight_forward"),
    ("mlp.hip", "launch_linear_t"): dict(entry=["pcl_linear_fwd_rows_f32", "pcl_linear_fwd_gmax_f32", "pcl_linear_bwd_dx_rows_f32",
                                                "pcl_linear_bwd_pair_f32", "pcl_mlp_stack_fwd_f32", "pcl_mlp_stack_bwd_f32"],
                                         external="x (layer 0), W; the running mean as mu in evaluation mode (the wrapper copies it)",
                                         misaligned="kernel: scalar staging (linear_nt_kernel<.., VEC = false>)", case=_MLP),
    ("mlp.hip", "pcl_linear_bwd_dw_rows_f32"): dict(entry=["pcl_linear_bwd_dw_rows_f32", "pcl_linear_bwd_dw_f32", "pcl_mlp_stack_bwd_f32"],
                                                    external="x (layer 0) as Xprev, features of a grouped stack; mu in evaluation mode",
                                                    misaligned="kernel: scalar staging (launch_dw_t<.., false>)", case=_MLP),
    ("mlp.hip", "pcl_linear_bwd_pair_f32"): dict(entry=["pcl_linear_bwd_pair_f32", "pcl_mlp_stack_bwd_f32"], external="x (layer 0), W",
                                                 misaligned="kernel: both bodies scalar, or the two plain launches when only one is", case="test_pointwise_mlp_few_rows"),
    ("mlp.hip", "pcl_bn_bwd_dy_f32"): dict(entry=["pcl_bn_bwd_dy_f32", "pcl_mlp_stack_bwd_f32"], external=_LIB, misaligned="error", case="test_pointwise_mlp_few_rows (gamma, the one caller's operand, goes by scalars)"),
    ("mlp.hip", "pcl_linear_bwd_dw_plain_f32"): dict(entry=["pcl_linear_bwd_dw_plain_f32", "pcl_mlp_stack_bwd_f32"], external="x (layer 0) as Xprev",
                                                     misaligned="kernel: scalar staging", case="test_pointwise_mlp_few_rows"),
    ("mlp.hip", "pcl_linear_bwd_fused_rows_f32"): dict(entry=["pcl_linear_bwd_fused_rows_f32"], external="W; mu in evaluation mode (the wrapper copies it)",
                                                       misaligned="error at the entry point; stack.hip and mlp_hip.py decline it for a misaligned W "
                                                                  "and run pcl_linear_bwd_dw_rows_f32 + pcl_linear_bwd_dx_rows_f32", case=_MLP + " / test_fused_backward_declines_by_launch_tags"),
    ("mlp.hip", "maxgrad_prep_impl"): dict(entry=["pcl_maxgrad_prep_f32", "pcl_maxgrad_prep_ld_f32", "pcl_mlp_stack_bwd_f32"], external=_LIB + " (the zero-fill region); gout goes by scalars",
                                           misaligned="error", case="test_pointwise_mlp_pooled (gout shifted and strided)"),
    ("stack.hip", "stack_bwd_impl"): dict(entry=["pcl_mlp_stack_bwd_f32"], external="W of a fused-backward layer; (dU of the folded layer: " + _LIB + ")",
                                          misaligned="kernel: the generic dW + dX launches instead of the fused backward",
                                          case=_MLP + " / test_fused_backward_declines_by_launch_tags"),
    ("frag.hip", "pcl_frag_dy_f32"): dict(entry=["pcl_frag_dy_f32"], external=_LIB + "; not called by the wrappers", misaligned="error",
                                          case="none (no caller's operand; the frag GEMMs take any 4-byte alignment by buffer loads, tests/test_frag_hip.py)"),
    ("compact.hip", "pcl_bn_act_max_rows_f32"): dict(entry=["pcl_bn_act_max_rows_f32", "pcl_mlp_stack_fwd_f32"], external=_LIB + " (Y); group_off goes by scalars",
                                                     misaligned="kernel: one channel per lane", case=_GRP),
    ("compact.hip", "group_linear_fwd_impl"): dict(entry=["pcl_group_linear_f32", "pcl_mlp_stack_fwd_f32"],
                                                   external=_LIB + " (Y, Uf); xyz, new_xyz, feature (<= 4 columns), W0, idx, cnt, group_off go by scalars",
                                                   misaligned="kernel: one channel per lane", case=_GRP),
    ("compact.hip", "group_linear_bwd_impl"): dict(entry=["pcl_group_linear_bwd_f32", "pcl_mlp_stack_bwd_f32"], external=_LIB + " (Y, dU)",
                                                   misaligned="kernel: one channel per lane", case=_GRP),
    ("compact.hip", "pcl_group_linear_bwd_gather_f32"): dict(entry=["pcl_group_linear_bwd_gather_f32"], external=_LIB, misaligned="error",
                                                             case="none (not called by the wrappers)"),
    ("compact.hip", "pcl_group_linear_bwd_regen_f32"): dict(entry=["pcl_group_linear_bwd_regen_f32", "pcl_mlp_stack_bwd_f32"], external=_LIB + "; W0 goes by scalars",
                                                            misaligned="error", case=_GRP),
    ("compact.hip", "pcl_group_linear_bwd_gather_regen_f32"): dict(entry=["pcl_group_linear_bwd_gather_regen_f32", "pcl_mlp_stack_bwd_f32"],
                                                                   external="mu in evaluation mode (the wrapper copies a misaligned running mean); W0 goes by scalars",
                                                                   misaligned="error", case=_GRP + " (evaluation mode)"),
    ("head.hip", "head_wide"): dict(entry=["pcl_head_layer_fwd_f32", "pcl_head_layer_bwd_f32", "pcl_fc_head_fwd_f32", "pcl_fc_head_bwd_f32"], external="x, W",
                                    misaligned="kernel: the one-column-per-workgroup kernels, which take 16-byte pieces only of aligned rows "
                                               "(head_vec_rows); dX stays on the MFMA kernel by size, its target cleared by the column kernel", case=_HEAD),
    ("head.hip", "head_layer_fwd_impl"): dict(entry=["pcl_head_layer_fwd_f32", "pcl_fc_head_fwd_f32"], external=_LIB + " (the split-K workspace)", misaligned="error", case=_HEAD),
    ("segpool.hip", "pcl_bn_act_seg_max_f32"): dict(entry=["pcl_bn_act_seg_max_f32"], external="Y, scale, shift", misaligned="kernel: one channel per lane",
                                                    case=_SEG),
    ("segpool.hip", "pcl_seg_broadcast_rows_f32"): dict(entry=["pcl_seg_broadcast_rows_f32"], external="src", misaligned="kernel: one float per piece", case=_SEG),
    ("pointconv.hip", "launch_bwd_w"): dict(entry=["pcl_pointconv_contract_bwd_f32", "pcl_pointconv_contract_bn_bwd_f32"], external="feat, dout (both required aligned by the entry points)",
                                            misaligned="kernel: the LDS-staged weight gradient (unreachable through the entry points' requirement)", case=_PC),
    ("pointconv.hip", "pcl_pointconv_contract_bwd_f32"): dict(entry=["pcl_pointconv_contract_bwd_f32"], external="dout, weights, feat (C % 4 == 0)",
                                                              misaligned="error; the wrapper copies a misaligned feat / weights / upstream gradient", case=_PC),
    ("pointconv.hip", "pcl_pointconv_contract_bn_bwd_f32"): dict(entry=["pcl_pointconv_contract_bn_bwd_f32"], external="dout, weights (Y, scale, shift: the deferring stack's)",
                                                                 misaligned="error; the wrapper copies misaligned weights / upstream gradient", case=_PC),
    ("xconv.hip", "pcl_xconv_core_bwd_f32"): dict(entry=["pcl_xconv_core_bwd_f32"], external="dD (depth_multiplier > 1)", misaligned="error; the wrapper copies a misaligned upstream gradient", case=_XC),
    ("knn.hip", "pcl_knn_point_matmul_f32"): dict(entry=["pcl_knn_point_matmul_f32"], external="xyz", misaligned="error (the documented requirement of knn_point(form='matmul'))", case=_KNN),
    ("head.hip", "head_vec_rows"): dict(entry=["pcl_head_layer_*", "pcl_fc_head_*"], external="x, W (in the column kernels, per workgroup)",
                                        misaligned="kernel: the same kernel's scalar loads", case=_HEAD),
    ("narrow.hip", "nw_bwd_kernel"): dict(entry=["pcl_mlp_stack_bwd_f32"], external="gout of a narrow stack (three layers of <= 16 channels, no input gradient)",
                                          misaligned="kernel: the same kernel's scalar loads", case="test_narrow_stack_gout"),
    ("mlp.hip", "linear_nt_body"): dict(entry=["the GEMM entry points"], external=_LIB + " (the output C, asked in the kernel)", misaligned="kernel: scalar stores",
                                        case="none (no caller's operand)"),
    ("mlp.hip", "linear_dw_body"): dict(entry=["the dW entry points"], external=_LIB + " (the partial tiles / dW, asked in the kernel)", misaligned="kernel: scalar stores",
                                        case="none (a caller's dW is a fresh gradient tensor or a piece of the stack's flat buffer: either way the kernel asks)"),
    ("pack.hip", "aligned8"): dict(entry=["pcl_fp_pack_rows_f32"], external="see pcl_fp_pack_rows_f32 (the predicate's definition)", misaligned="kernel: one float per piece",
                                   case="test_interpolate_pack"),
    ("pack.hip", "pcl_fp_pack_rows_f32"): dict(entry=["pcl_fp_pack_rows_f32"], external="points2 (8 bytes); rows is the operator's own allocation", misaligned="kernel: one float per piece",
                                               case="test_interpolate_pack"),
    ("sgd.hip", "sgd_momentum_kernel"): dict(entry=["pcl_sgd_momentum_f32"], external="parameters, gradients, momentum buffers (asked per tensor in the kernel)",
                                             misaligned="kernel: the same kernel's scalar loads", case="tests/test_sgd_gpu.py (every residue of every tensor)"),
    ("infer.hip", "sa_level_infer"): dict(entry=["pcl_sa_level_infer_f32", "pcl_sa_level_infer_bf16"], external=_FROZEN, misaligned="error", case="none"),
    ("infer_fp.hip", "fp_run"): dict(entry=["pcl_fp_level_infer_f32", "pcl_fp_level_infer_bf16"], external=_FROZEN, misaligned="error", case="none"),
    ("infer_pointnet.hip", "pn_stack_infer"): dict(entry=["pcl_pointnet_stack_infer_f32", "pcl_pointnet_stack_infer_bf16"], external=_FROZEN, misaligned="error", case="none"),
    ("infer_pointnet_seg.hip", "seg_part_ok"): dict(entry=["pcl_pointnet_seg_*_infer_f32"], external=_FROZEN, misaligned="error", case="none"),
    ("infer_pointnet_seg.hip", "seg_rows_ok"): dict(entry=["pcl_pointnet_seg_*_infer_f32"], external=_FROZEN, misaligned="error", case="none"),
    ("infer_pointnet_seg.hip", "seg_front_infer"): dict(entry=["pcl_pointnet_seg_stn_infer_f32", "pcl_pointnet_seg_trunk_infer_f32"], external=_FROZEN, misaligned="error", case="none"),
    ("infer_pointnet_seg.hip", "seg_global_infer"): dict(entry=["pcl_pointnet_seg_global_infer_f32", "pcl_pointnet_seg_global_infer_bf16_f32"], external=_FROZEN, misaligned="error", case="none"),
    ("infer_pointnet_seg.hip", "seg_head_infer"): dict(entry=["pcl_pointnet_seg_head_infer_f32", "pcl_pointnet_seg_head_infer_bf16_f32"], external=_FROZEN, misaligned="error", case="none"),
    ("infer_pointnet_seg.hip", "pcl_pointnet_seg_rows_f32"): dict(entry=["pcl_pointnet_seg_rows_f32"], external=_FROZEN, misaligned="error", case="none"),
}


# ---- shared helpers ---------------------------------------------------------------------------------------------------------------
def _err(a, b64):
    return (a.detach().double().cpu() - b64.detach().double().cpu()).abs().max().item()


def _mis(t):
    assert t.data_ptr() % 16 != 0, "the operand under test is aligned"
    return t


@contextlib.contextmanager
def _path(stack):
    """the per-stack entry points (the default) or the per-kernel path"""
    from pointcloudlib_amd.misc import mlp_hip
    if stack:
        yield
    else:
        with mlp_hip.per_kernel_path():
            yield


def _shift_mlp(m, which, k):
    """move a class of a PointwiseMLP's tensors in place (the Parameter / buffer objects stay)"""
    if which in ("W", "all"):
        for i, w in enumerate(m.weights):
            w.data = shifted(w.data, (k + i - 1) % 3 + 1)
    if which in ("bn", "all"):
        for lst in (m.gammas, m.betas, m.biases):
            for i, p in enumerate(lst if lst is not None else []):
                p.data = shifted(p.data, (k + i) % 3 + 1)
    if which in ("running", "all"):
        for i, (n, b) in enumerate(m.named_buffers()):
            b.data = shifted(b.data, (k + i + 1) % 3 + 1)


def _mlp64(spec, bias, slope, seed):
    torch.manual_seed(seed)
    m = PointwiseMLP(spec, bias=bias, slope=slope).double()
    with torch.no_grad():
        for g, b in zip(m.gammas, m.betas):
            g.uniform_(0.5, 1.5); b.uniform_(-0.3, 0.3)
            g[::3] *= -1.0
        for n, b in m.named_buffers():                # evaluation mode reads them: not the initial 0 / 1
            b.copy_(torch.randn_like(b) * 0.3 if "mean" in n else torch.empty_like(b).uniform_(0.5, 1.5))
    return m


def _run_mlp(m, x, ns, gout, backend, training):
    """forward + backward WITHOUT moving x or gout (a clone would be a fresh, aligned allocation)"""
    m.backend = backend
    m.train(training)
    m.zero_grad()
    xx = x.detach().requires_grad_(True)
    assert xx.data_ptr() == x.data_ptr()
    out = m(xx, group_max=ns)
    out.backward(gout)
    return (out.detach(), xx.grad.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()},
            {n: b.detach().clone() for n, b in m.named_buffers()})


def _check_mlp_fp64(tag, got, t32, ref, training):
    """the rule of tests/test_mlp_hip.py::_check_against_fp64: features and running statistics within 1e-5 * max(1, |ref|_max); gradients within
    1e-4 of the gradient's max-norm, or 4x the error of PyTorch's own fp32 GPU path against the same fp64 truth"""
    scale = max(1.0, ref[0].abs().max().item())
    e = _err(got[0], ref[0])
    assert e <= 1e-5 * scale, f"{tag}: features {e:.3e}, scale {scale:.3f}"
    gs = max(1e-6, ref[1].abs().max().item())
    e, e_t = _err(got[1], ref[1]), _err(t32[1], ref[1])
    assert e <= max(1e-4 * gs, 4 * e_t), f"{tag}: input grad {e:.3e} (torch fp32 {e_t:.3e}), scale {gs:.3e}"
    for n in ref[2]:
        if "biases" in n and training:                # the bias feeds BatchNorm: the true gradient is 0
            assert got[2][n].abs().max().item() <= 1e-4, f"{tag}: {n}"
            continue
        gs = max(1e-6, ref[2][n].abs().max().item())
        e, e_t = _err(got[2][n], ref[2][n]), _err(t32[2][n], ref[2][n])
        assert e <= max(1e-4 * gs, 4 * e_t), f"{tag}: {n} {e:.3e} (torch fp32 {e_t:.3e}), scale {gs:.3e}"
    for n in ref[3]:
        e = _err(got[3][n], ref[3][n])
        assert e <= 1e-5 * max(1.0, ref[3][n].abs().max().item()), f"{tag}: {n} {e:.3e}"


# Per family, the operand classes whose move changes NO kernel (every kernel reads them by scalars, or the wrapper copies them): those runs are
# bit-equal to the aligned run.  The others change a kernel (the table's "misaligned ->" column).
SAME_KERNELS = {"mlp": {"bn", "running", "gout"},
                "grouped": {"xyz", "new_xyz", "feature", "idx", "cnt", "group_off", "gout", "bn", "running"},
                "head": {"vectors", "running", "gout"}}


def _against_aligned(tag, got, base, same):
    """bit-equal where the same kernels run; else the largest difference is printed and held to the op's fp64 bound: features and running
    statistics 1e-5 * max(1, |aligned|_max), gradients 1e-4 of the gradient's max-norm (the part of tests/test_mlp_hip.py's gradient rule that needs
    no second reference), a bias gradient under training-mode BatchNorm (true value 0) 1e-4 absolute"""
    flat_g = [("out", got[0]), ("dx", got[1])] + sorted(got[2].items()) + sorted(got[3].items())
    flat_b = [("out", base[0]), ("dx", base[1])] + sorted(base[2].items()) + sorted(base[3].items())
    worst = ("", 0.0)
    for (n, a), (_, b) in zip(flat_g, flat_b):
        if a is None:
            continue
        if same:
            assert torch.equal(a, b), f"{tag}: {n} differs from the aligned run ({(a - b).abs().max().item():.3e}) although the same kernels run"
            continue
        d, sc = (a - b).abs().max().item(), b.abs().max().item()
        worst = max(worst, (n, d / max(1e-30, sc)), key=lambda t: t[1])
        if n == "out" or n.startswith("running"):
            bound = 1e-5 * max(1.0, sc)
        elif "biases" in n:
            bound = max(1e-4, 1e-4 * sc)
        else:
            bound = 1e-4 * max(1e-6, sc)
        assert d <= bound, f"{tag}: {n} is {d:.3e} from the aligned run, bound {bound:.3e}"
    if not same:
        print(f"{tag}: largest difference to the aligned run {worst[1]:.3e} of the tensor's max-norm ({worst[0]})")


# evaluation mode has one host path (the per-stack entry points take training-mode BatchNorm only)
MODES = [pytest.param(True, True, id="train-stack"), pytest.param(True, False, id="train-per-kernel"), pytest.param(False, False, id="eval")]
_MLP_VARIANTS = [(w, w in SAME_KERNELS["mlp"]) for w in ("x", "W", "bn", "running", "gout", "all")]      # (operand class, same kernels)


def _mlp_sweep(dev, spec, lead, ns, bias, slope, training, stack, gout_of=None):
    """(a) aligned, (b) one class shifted, (c) all shifted; ``gout_of``: maps the dense fp32 gout to the tensor handed to backward"""
    m64 = _mlp64(spec, bias, slope, 1234 + spec[0] + (ns or 0))
    x64 = torch.randn(*lead, spec[0], dtype=torch.float64)
    if ns:
        x64[..., ns // 2:, :] = x64[..., :1, :]        # padded duplicates inside groups (ball-query padding): ties of the max
    gout64 = torch.randn((*lead[:-1], spec[-1]) if ns else (*lead, spec[-1]), dtype=torch.float64)
    ref = _run_mlp(copy.deepcopy(m64), x64, ns, gout64, "torch", training)
    m32 = copy.deepcopy(m64).float().to(dev)
    x32, g32 = x64.float().to(dev), gout64.float().to(dev)
    t32 = _run_mlp(copy.deepcopy(m32), x32, ns, g32, "torch", training)
    name = f"{spec} {lead} ns={ns} {'train' if training else 'eval'} {'stack' if stack else 'per-kernel'}"
    with _path(stack):
        g_al = g32 if gout_of is None else gout_of(g32, 0)
        base = _run_mlp(copy.deepcopy(m32), x32, ns, g_al, "hip", training)
        _check_mlp_fp64(f"{name} aligned", base, t32, ref, training)
        for k, (which, same) in enumerate(_MLP_VARIANTS, start=1):
            m = copy.deepcopy(m32)
            _shift_mlp(m, which, k)
            x = _mis(shifted(x32, (k - 1) % 3 + 1)) if which in ("x", "all") else x32
            g = g_al
            if which in ("gout", "all"):
                g = _mis(shifted(g32, k % 3 + 1)) if gout_of is None else gout_of(g32, k % 3 + 1)
            got = _run_mlp(m, x, ns, g, "hip", training)          # must not raise
            _check_mlp_fp64(f"{name} {which} shifted", got, t32, ref, training)
            _against_aligned(f"{name} {which} shifted", got, base, same)


# ---- PointwiseMLP, plain rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training,stack", MODES)
@pytest.mark.parametrize("spec,rows", [([16, 64, 128, 64], 3333),       # the fused backward at 128 x 64 and 64 x 128
                                       ([12, 128, 128], 4097), ([8, 64, 64], 4097)])
def test_pointwise_mlp_plain_rows(dev, spec, rows, training, stack):
    _mlp_sweep(dev, spec, (rows,), None, True, 0.2, training, stack)


@pytest.mark.parametrize("stack", [True, False], ids=["stack", "per-kernel"])
def test_resident_weight_forward(dev, stack):
    """fwd_res_eligible takes >= 32768 rows: [64, 64, 128] with biases on 32801 rows, both layers of resident-weight shape, forward only (at this
    size an fp64 comparison of the gradients meets ReLU-mask flips, tests/test_mlp_hip.py::test_fused_backward_tiles_per_block).  Features and
    running statistics against fp64 under test_resident_weight_forward_kernel_against_fp64's bound, 1e-5 * max(1, |ref|_max), aligned and with
    W / bias / x moved.  The fp32 kernel reads X and W through 16-byte buffer loads (any 4-byte alignment) and the bias by scalars, so every moved
    run keeps the kernel and is bit-equal to the aligned one."""
    from pointcloudlib_amd import _lib
    spec, rows = [64, 64, 128], 32801
    m64 = _mlp64(spec, True, 0.0, 77)
    x64 = torch.randn(rows, spec[0], dtype=torch.float64)
    with torch.no_grad():
        m64.backend = "torch"; m64.train()
        bufs0 = {n: b.clone() for n, b in m64.named_buffers()}
        want = m64(x64)
        bufs = {n: b.clone() for n, b in m64.named_buffers()}
        for n, b in m64.named_buffers():
            b.copy_(bufs0[n])
    m32, x32 = copy.deepcopy(m64).float().to(dev), x64.float().to(dev)
    seen, outs = {}, {}
    for which in ("aligned", "W", "bn", "x"):
        m = copy.deepcopy(m32).train()
        m.backend = "hip"
        if which != "aligned":
            _shift_mlp(m, which, 2)
        x = _mis(shifted(x32, 1)) if which == "x" else x32
        with torch.no_grad(), _path(stack):
            got = m(x)
        e = _err(got, want)
        assert e <= 1e-5 * max(1.0, want.abs().max().item()), f"{which}: features {e:.3e}"
        for n, b in m.named_buffers():
            assert _err(b, bufs[n]) <= 1e-5 * max(1.0, bufs[n].abs().max().item()), f"{which}: {n}"
        outs[which] = (got, {n: b.detach().clone() for n, b in m.named_buffers()})
        if not stack:                          # which kernel each forward call chose (the per-kernel path: one C call per layer)
            timer = _lib.KernelTimer(names=["pcl_linear_fwd_rows_f32"])
            _lib.PROFILER = timer
            try:
                with torch.no_grad(), _path(False):
                    m(x)                           # (m itself: a deep copy would be a fresh, aligned allocation)
                torch.cuda.synchronize()
            finally:
                _lib.PROFILER = None
            seen[which] = [(tag, fam) for _, tag, fam in timer.order]
    for which in ("W", "bn", "x"):
        assert torch.equal(outs[which][0], outs["aligned"][0]), f"{which} moved: the forward differs from the aligned run"
        for n, b in outs[which][1].items():
            assert torch.equal(b, outs["aligned"][1][n]), f"{which} moved: {n}"
    if not stack:
        print("kernels of the forward:", seen)
        res = [("fwd64x64", "linear_fwd_res_kernel"), ("fwd64x128", "linear_fwd_res_kernel")]
        assert seen["aligned"] == seen["W"] == seen["bn"] == seen["x"] == res, seen


@pytest.mark.parametrize("stack", [True, False], ids=["stack", "per-kernel"])
@pytest.mark.parametrize("which", ["fewrow", "pair"])
def test_pointwise_mlp_few_rows(dev, which, stack):
    """The smallest shapes at which the two few-row backward forms answer 1.  pcl_mlp_fewrow_layer (behind pcl_set_fewrow_backward(1)): any P >= 1
    with Cout a multiple of 32 and no fused backward for the shape -> [12, 32, 32] on 33 rows.  pcl_linear_bwd_pair_supported: Cout, Cin > 64 (it answers by the sizes of
    the two GEMMs, also 1 for the fused backward's 128 x 128 and 256 x 128, where the stack asks it only if the fused kernel does not run) -> 96 x 96 ([12, 96, 96] on 33 rows; per-stack path only, the per-kernel path runs the two launches)."""
    from pointcloudlib_amd import _lib
    L = _lib.lib()
    spec = [12, 32, 32] if which == "fewrow" else [12, 96, 96]
    prev = L.pcl_get_fewrow_backward()
    try:
        if which == "fewrow":
            L.pcl_set_fewrow_backward(1)
            assert L.pcl_mlp_fewrow_layer(33, 32, 32, 0) == 1 and L.pcl_mlp_fewrow_layer(33, 32, 12, 1) == 1
        else:
            assert L.pcl_linear_bwd_pair_supported(33, 96, 96, 0) == 1 and L.pcl_linear_bwd_pair_supported(33, 96, 12, 0) == 0
        _mlp_sweep(dev, spec, (33,), None, True, 0.0, True, stack)
    finally:
        L.pcl_set_fewrow_backward(prev)


# ---- pooled PointwiseMLP ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training,stack", MODES)
@pytest.mark.parametrize("ns", [32, 16])
def test_pointwise_mlp_pooled(dev, ns, training, stack):
    _mlp_sweep(dev, [16, 64, 128, 64], (2, 40, ns), ns, False, 0.0, training, stack)


@pytest.mark.parametrize("ns", [32, 16])
@pytest.mark.parametrize("col,width,total", [(3, 30, 37), (64, 128, 197)])
def test_pointwise_mlp_pooled_strided_gout(dev, ns, col, width, total):
    """gout as an in-place column slice of a wider gradient whose width is no multiple of 4 (rows at every residue), itself at an odd offset in
    the shifted runs: the max-gradient kernel reads it by scalars with its row stride, no copy (COUNTERS)."""
    from pointcloudlib_amd.misc import mlp_hip

    def gout_of(g32, k):
        wide = torch.randn(*g32.shape[:-1], total, device=g32.device)
        wide = shifted(wide, k) if k else wide
        wide[..., col:col + width] = g32
        return wide[..., col:col + width]

    n0 = mlp_hip.COUNTERS["strided_gout"]
    _mlp_sweep(dev, [16, 64, width], (2, 40, ns), ns, False, 0.0, True, True, gout_of=gout_of)
    assert mlp_hip.COUNTERS["strided_gout"] == n0 + 1 + len(_MLP_VARIANTS), "a strided gout was copied instead of read in place"


# ---- the fused backward declines by alignment: launch tags --------------------------------------------------------------------------
def test_fused_backward_declines_by_launch_tags(dev):
    """[16, 64, 128, 64] on 3333 rows.  Aligned: the backward's GEMM launches are the ones the size rule alone selects (fused 64 x 128 and
    128 x 64, dW + dX for the 16-wide first layer) on both host paths.  W[2] moved: that layer -- and only that one -- runs
    pcl_linear_bwd_dw_rows_f32 + pcl_linear_bwd_dx_rows_f32 (tags dw64x128, dx64x128), on both paths."""
    from pointcloudlib_amd import _lib
    spec, rows = [16, 64, 128, 64], 3333
    torch.manual_seed(5)
    m0 = PointwiseMLP(spec).to(dev).train()
    x = torch.randn(rows, spec[0], device=dev)
    gout = torch.randn(rows, spec[-1], device=dev)
    gemm = {"pcl_linear_bwd_fused_rows_f32", "pcl_linear_bwd_dw_rows_f32", "pcl_linear_bwd_dx_rows_f32", "pcl_linear_bwd_pair_f32",
            "pcl_linear_bwd_dw_plain_f32", "pcl_frag_linear_bwd_dx_f32"}
    want = {False: [("pcl_linear_bwd_fused_rows_f32", "fb64x128"), ("pcl_linear_bwd_fused_rows_f32", "fb128x64"),
                    ("pcl_linear_bwd_dw_rows_f32", "dw64x16"), ("pcl_linear_bwd_dx_rows_f32", "dx64x16")],
            True: [("pcl_linear_bwd_dw_rows_f32", "dw64x128"), ("pcl_linear_bwd_dx_rows_f32", "dx64x128"), ("pcl_linear_bwd_fused_rows_f32", "fb128x64"),
                   ("pcl_linear_bwd_dw_rows_f32", "dw64x16"), ("pcl_linear_bwd_dx_rows_f32", "dx64x16")]}
    res = {}
    for moved in (False, True):
        m = copy.deepcopy(m0)
        if moved:
            m.weights[2].data = _mis(shifted(m.weights[2].data, 1))
        # the per-kernel path: every C call in order
        timer = _lib.KernelTimer()
        _lib.PROFILER = timer
        try:
            with _path(False):
                res[(moved, False)] = _run_mlp(m, x, None, gout, "hip", True)          # (m itself: a deep copy would be a fresh, aligned allocation)
            torch.cuda.synchronize()
        finally:
            _lib.PROFILER = None
        with _path(True):
            for n, b in m.named_buffers():
                b.copy_(dict(m0.named_buffers())[n])           # (the running statistics the first run moved: both paths start from the same)
            res[(moved, True)] = _run_mlp(m, x, None, gout, "hip", True)
        got = [(n, t) for n, t, _ in timer.order if n in gemm]
        assert got == want[moved], (moved, got)
        # the per-stack path: which launch tags occur inside pcl_mlp_stack_bwd_f32
        seen = {}
        for tag in ("fb64x128", "fb128x64", "dw64x128", "dx64x128", "dw128x64", "dx128x64", "dw64x16", "dx64x16", "pair64x128"):
            timer = _lib.KernelTimer(inner=("pcl_mlp_stack_bwd_f32", tag, 0, 0))
            _lib.PROFILER = timer
            try:
                with _path(True):
                    _run_mlp(m, x, None, gout, "hip", True)
                torch.cuda.synchronize()
            finally:
                _lib.PROFILER = None
            seen[tag] = timer.summary().get(("pcl_mlp_stack_bwd_f32", tag), {}).get("launches", 0)
        launched = sorted(t for t, n in seen.items() if n)
        assert launched == sorted(t for _, t in want[moved]), (moved, seen)
    # the mixed order (layer 2 on dW + dX, the fused kernel for layer 1 below it) computes the same step: both host paths bit-equal to each
    # other, and within the fp64 bound of the aligned run (forward and running statistics: the same kernels, bit-equal)
    for moved in (False, True):
        _against_aligned(f"W[2] moved={moved}: per-stack against per-kernel path", res[(moved, True)], res[(moved, False)], True)
    for stack in (False, True):
        _against_aligned(f"W[2] moved, stack={stack}", res[(True, stack)], res[(False, stack)], False)
        assert torch.equal(res[(True, stack)][0], res[(False, stack)][0])
        for n in res[(True, stack)][3]:
            assert torch.equal(res[(True, stack)][3][n], res[(False, stack)][3][n]), n


# ---- forward_grouped ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training,stack", MODES)
@pytest.mark.parametrize("C", [13, 0])
def test_forward_grouped(dev, C, training, stack):
    """B = 2, N = 256, m = 32, ns = 16, spec [3 + C, 64, 128] (C = 13: [16, 64, 128]; C = 0: coordinates only), against the fp64 composite on
    rows gathered with the same indices, under the rule of tests/test_mlp_hip.py.  Every external operand goes by scalars (INVENTORY): moved xyz,
    new_xyz, feature, idx, cnt, group_off and BatchNorm vectors select the same kernels -- bit-equal except, with wide features, what the
    fp32 atomics of the per-kernel path's scatter touch; a moved W changes the staging of the layers behind the folded one."""
    from pointcloudlib_amd import synth
    from pointcloudlib_amd.misc import ops
    B, N, m_, ns = 2, 256, 32, 16
    spec = [3 + C, 64, 128]
    xyz = torch.from_numpy(synth.gauss_ball(B, N, 31)).to(dev)
    torch.manual_seed(40 + C)
    feat = torch.randn(B, N, C, device=dev) if C else None
    _, new_xyz = ops.furthest_point_sample(xyz, m_)
    idx, cnt = ops.ball_query(new_xyz, xyz, 0.35, ns, return_cnt=True)
    goff = ops.group_offsets(cnt)
    m64 = _mlp64(spec, False, 0.0, 90 + C)
    gout64 = torch.randn(B, m_, spec[-1], dtype=torch.float64)

    def reference(mod, dtype, device):
        """the composite on rows gathered with the same (padded) indices: [xyz[idx] - new_xyz | feature[idx]]"""
        mod.backend = "torch"; mod.train(training); mod.zero_grad()
        ii = idx.to(device).long()
        bi = torch.arange(B, device=device)[:, None, None]
        f = None if feat is None else feat.detach().to(device=device, dtype=dtype).requires_grad_(True)
        rows = xyz.to(device=device, dtype=dtype)[bi, ii] - new_xyz.to(device=device, dtype=dtype)[:, :, None, :]
        if f is not None:
            rows = torch.cat((rows, f[bi, ii]), dim=-1)
        out = mod(rows, group_max=ns)
        out.backward(gout64.to(device=device, dtype=dtype))
        return (out.detach(), None if f is None else f.grad.detach(), {n: p.grad.detach().clone() for n, p in mod.named_parameters()},
                {n: b.detach().clone() for n, b in mod.named_buffers()})

    ref = reference(copy.deepcopy(m64), torch.float64, "cpu")
    m32 = copy.deepcopy(m64).float().to(dev)
    t32 = reference(copy.deepcopy(m32), torch.float32, dev)
    g32 = gout64.float().to(dev)

    def run(mod, ops_):
        mod.backend = "hip"; mod.train(training); mod.zero_grad()
        f = None if ops_["feature"] is None else ops_["feature"].detach().requires_grad_(True)
        out = mod.forward_grouped(ops_["xyz"], ops_["new_xyz"], f, ops_["idx"], ops_["cnt"], ops_["group_off"], True)
        out.backward(ops_["gout"])
        return (out.detach(), None if f is None else f.grad.detach(), {n: p.grad.detach().clone() for n, p in mod.named_parameters()},
                {n: b.detach().clone() for n, b in mod.named_buffers()})

    def check(tag, got):
        fixed = (got[0], got[1] if got[1] is not None else torch.zeros(1), got[2], got[3])
        r = (ref[0], ref[1] if ref[1] is not None else torch.zeros(1), ref[2], ref[3])
        t = (t32[0], t32[1] if t32[1] is not None else torch.zeros(1), t32[2], t32[3])
        _check_mlp_fp64(tag, fixed, t, r, training)

    aligned = dict(xyz=xyz, new_xyz=new_xyz, feature=feat, idx=idx, cnt=cnt, group_off=goff, gout=g32)
    name = f"grouped C={C} {'train' if training else 'eval'} {'stack' if stack else 'per-kernel'}"
    atomics = C > 4 and not stack          # the per-kernel path's scatter to the points adds with fp32 atomics (arrival order)
    with _path(stack):
        base = run(copy.deepcopy(m32), aligned)
        check(f"{name} aligned", base)
        variants = ["xyz", "new_xyz", "idx", "cnt", "group_off", "gout", "bn", "running", "W", "all"] + (["feature"] if C else [])
        for k, which in enumerate(variants, start=1):
            o = dict(aligned)
            mod = copy.deepcopy(m32)
            for key in o:
                if o[key] is not None and which in (key, "all"):
                    o[key] = _mis(shifted(o[key], (k + len(key)) % 3 + 1))
            if which in ("bn", "running", "W", "all"):
                _shift_mlp(mod, which, k)
            got = run(mod, o)                  # must not raise
            check(f"{name} {which} shifted", got)
            same = which in SAME_KERNELS["grouped"] and not atomics          # (a moved feature: K = 13 is staged by scalars either way)
            _against_aligned(f"{name} {which} shifted", got, base, same)


# ---- fc_head ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stack", [True, False], ids=["stack", "per-layer"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("spec,R", [([2048, 64, 10], 8), ([64, 40, 10], 33), ([2048, 512, 40], 32)])
def test_fc_head(dev, spec, R, training, stack):
    """[Linear -> BatchNorm1d -> ReLU] x (L - 1) -> Linear against the PyTorch modules in fp64 under test_head_layer_matches_torch's bound,
    2e-5 * max(1, |ref|_max), for the logits, every gradient and the running statistics (running_var by Jittor's rule, biased variance: redone in the
    reference as there).  [2048, 64, 10] on 8 rows is a wide-path candidate (head_wide): x and W are moved separately."""
    from pointcloudlib_amd.misc import head
    torch.manual_seed(R + spec[0])
    mods = []
    for i in range(len(spec) - 1):
        last = i == len(spec) - 2
        mods.append(nn.Linear(spec[i], spec[i + 1], bias=last))
        if not last:
            mods += [nn.BatchNorm1d(spec[i + 1]), nn.ReLU()]
    seq64 = nn.Sequential(*mods).double()
    with torch.no_grad():
        for mod in seq64:
            if isinstance(mod, nn.BatchNorm1d):
                mod.weight.uniform_(-1.0, 1.5); mod.bias.uniform_(-0.5, 0.5)
                mod.running_mean.normal_(0.0, 0.3); mod.running_var.uniform_(0.5, 1.5)
    x64 = torch.randn(R, spec[0], dtype=torch.float64)
    g64 = torch.randn(R, spec[-1], dtype=torch.float64)
    # the fp64 truth, with running_var redone with the biased batch variance
    r = copy.deepcopy(seq64).train(training)
    rv0 = {i: mod.running_var.clone() for i, mod in enumerate(r) if isinstance(mod, nn.BatchNorm1d)}
    xr = x64.clone().requires_grad_(True)
    h, pre = xr, {}
    for i, mod in enumerate(r):
        if isinstance(mod, nn.BatchNorm1d):
            pre[i] = h.detach()
        h = mod(h)
    h.backward(g64)
    if training:
        with torch.no_grad():
            for i, mod in enumerate(r):
                if isinstance(mod, nn.BatchNorm1d):
                    mod.running_var.copy_(rv0[i] + (pre[i].var(dim=0, unbiased=False) - rv0[i]) * mod.momentum)
    want = {"out": h.detach(), "dx": xr.grad, **{n: p.grad for n, p in r.named_parameters()},
            **{n: b for n, b in r.named_buffers() if b.dtype == torch.float64}}
    seq32 = copy.deepcopy(seq64).float().to(dev)
    x32, g32 = x64.float().to(dev), g64.float().to(dev)

    def run(seq, x, g):
        seq.train(training); seq.zero_grad()
        xx = x.detach().requires_grad_(True)
        out = head.fc_head(seq, xx)
        out.backward(g)
        return {"out": out.detach(), "dx": xx.grad, **{n: p.grad for n, p in seq.named_parameters()},
                **{n: b.detach().clone() for n, b in seq.named_buffers() if b.dtype == torch.float32}}

    def check(tag, got):
        for n, w in want.items():
            e = _err(got[n], w)
            assert e <= 2e-5 * max(1.0, w.abs().max().item()), f"{tag}: {n} {e:.3e}"

    old = head.USE_STACK
    head.USE_STACK = stack
    try:
        name = f"head {spec} R={R} {'train' if training else 'eval'} {'stack' if stack else 'per-layer'}"
        base = run(copy.deepcopy(seq32), x32, g32)
        check(f"{name} aligned", base)
        for k, which in enumerate(["x", "W", "vectors", "running", "gout", "all"], start=1):
            seq = copy.deepcopy(seq32)
            for j, (n, p) in enumerate(list(seq.named_parameters()) + list(seq.named_buffers())):
                if p.dtype != torch.float32:
                    continue
                kind = "W" if p.dim() == 2 else ("running" if "running" in n else "vectors")
                if which in (kind, "all"):
                    p.data = _mis(shifted(p.data, (k + j) % 3 + 1))
            x = _mis(shifted(x32, k % 3 + 1)) if which in ("x", "all") else x32
            g = _mis(shifted(g32, (k + 1) % 3 + 1)) if which in ("gout", "all") else g32
            got = run(seq, x, g)                   # must not raise
            check(f"{name} {which} shifted", got)
            # vectors, running statistics and gout go by scalars in every kernel: the same kernels run.  (dX of a K >= 2048 layer on <= 32 rows
            # adds with fp32 atomics: x.grad is compared by the fp64 bound only.)
            same = which in SAME_KERNELS["head"]
            worst = 0.0
            for n in base:
                if same and not (n == "dx" and spec[0] >= 2048 and R <= 32):
                    assert torch.equal(got[n], base[n]), f"{name} {which} shifted: {n} differs from the aligned run although the same kernels run"
                d, sc = (got[n] - base[n]).abs().max().item(), base[n].abs().max().item()
                assert d <= 2e-5 * max(1.0, sc), f"{name} {which} shifted: {n} is {d:.3e} from the aligned run, bound {2e-5 * max(1.0, sc):.3e}"
                worst = max(worst, d / max(1e-30, sc))
            if not same:
                print(f"{name} {which} shifted: largest difference to the aligned run {worst:.3e} of the tensor's max-norm")
    finally:
        head.USE_STACK = old


# ---- segmented pooling ----------------------------------------------------------------------------------------------------------------
def test_segment_pooling(dev):
    """ops.segment_max (pcl_bn_act_seg_max_f32 + bwd) and ops.broadcast_rows (pcl_seg_broadcast_rows_f32, backward pcl_seg_sum_rows_f32) on B = 3 clouds
    of 5, 64 and 17 rows, C = 64.  Bounds of tests/test_segpool_gpu.py: the max is a selection of fmaf + lrelu values -- within 1 ulp of the fp64
    value of the winner (two roundings: the fmaf and the product with the slope, which the reference takes as the same fp32 number) and no ties
    in random rows; du is gout or gout * slope, one rounding; the broadcast is a copy (exact); the segment sum is within
    2^-24 |s| + n_b 2^-52 sum|g| of the fp64 sum s.  The vector and the scalar kernels compute the same expression per element: moved operands
    give bit-equal results."""
    from pointcloudlib_amd.misc import ops
    lengths, C = [5, 64, 17], 64
    B, R = len(lengths), sum(lengths)
    row_off, _ = ops.row_offsets(lengths, B, max(lengths), dev)
    rc = ops.row_cloud(row_off, B, R)
    off = row_off.tolist()
    g = torch.Generator().manual_seed(3)
    Y = torch.randn(R, C, generator=g).to(dev)
    scale = (torch.randn(C, generator=g).abs() + 0.5) * torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)
    scale, shift = scale.to(dev), (0.3 * torch.randn(C, generator=g)).to(dev)
    gout = torch.randn(B, C, generator=g).to(dev)
    src = torch.randn(B, C, generator=g).to(dev)
    grows = torch.randn(R, C, generator=g).to(dev)
    slope = float(torch.tensor(0.2, dtype=torch.float32))       # the fp32 number the kernel multiplies by

    def run(o):
        y = o["Y"].detach().requires_grad_(True)
        out = ops.segment_max(y, o["row_off"], o["rc"], B, scale=o["scale"], shift=o["shift"], slope=slope)
        out.backward(o["gout"])
        v = o["src"].detach().requires_grad_(True)
        rows = ops.broadcast_rows(v, o["row_off"], o["rc"], R)
        rows.backward(o["grows"])
        return out.detach(), y.grad, rows.detach(), v.grad

    aligned = dict(Y=Y, scale=scale, shift=shift, gout=gout, src=src, grows=grows, row_off=row_off, rc=rc)
    base = run(aligned)
    # fp64 truth
    # (what the operator hands back for Y is du, the gradient w.r.t. u = scale * y + shift: scale / shift are constants of the pooling)
    u64 = (scale.double().cpu() * Y.double().cpu() + shift.double().cpu()).requires_grad_(True)
    z = torch.nn.functional.leaky_relu(u64, slope)
    want = torch.stack([z[off[b]:off[b + 1]].max(0)[0] for b in range(B)])
    want.backward(gout.double().cpu())
    assert _err(base[0], want) <= 2.0 ** -23 * max(1.0, z.detach().abs().max().item())     # two roundings of at most 2^-24 |value| each
    assert _err(base[1], u64.grad) <= 2.0 ** -24 * max(1.0, u64.grad.abs().max().item())   # one rounding
    assert torch.equal(base[2], src[rc.long()])
    g64 = grows.double().cpu()
    for b in range(B):
        seg = g64[off[b]:off[b + 1]]
        s = seg.sum(0)
        bound = 2.0 ** -24 * s.abs() + lengths[b] * 2.0 ** -52 * seg.abs().sum(0)
        assert bool(((base[3][b].double().cpu() - s).abs() <= bound).all()), f"segment sum, cloud {b}"
    for k, which in enumerate(["Y", "scale", "shift", "gout", "src", "grows", "row_off", "rc", "all"], start=1):
        o = dict(aligned)
        for j, key in enumerate(o):
            if which in (key, "all"):
                o[key] = _mis(shifted(o[key], (k + j) % 3 + 1))
        got = run(o)                           # must not raise
        for n, a, b_ in zip(("max", "dY", "rows", "dsrc"), got, base):
            assert torch.equal(a, b_), f"segment pooling, {which} shifted: {n} differs from the aligned run"


# ---- PointConv's contraction ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("folded", [False, True], ids=["plain", "folded-bn"])
def test_pointconv_contract(dev, folded):
    """G = 6 groups (B = 2, S = 3), ns = 16, C = 64, M = 16, forward and backward, against the reference formula in fp64 under
    test_pointconv_contraction_kernel's bound, 1e-5 * max(1, |ref|_max).  ``folded``: the feature MLP's last BatchNorm + activation inside the contraction
    (feature_mlp_contract on a [8, 64] stack): everything then went through the stack and is held to the gradient rule of tests/test_mlp_hip.py
    (1e-4 of the tensor's max-norm, or 4x the error of PyTorch's fp32 pipeline against the same truth), the running statistics to 1e-5.
    The wrapper copies a misaligned feat / weights / upstream gradient (the backward kernels move 16-byte pieces of them); density goes by
    scalars: every moved run selects the same kernels on the same values -- bit-equal."""
    from pointcloudlib_amd.misc.pointconv_utils import feature_mlp_contract, pointconv_contract
    B, S, ns, C = 2, 3, 16, 64
    torch.manual_seed(ns + C)
    d64 = torch.rand(B, S, ns, 1, dtype=torch.float64) + 0.1
    w64 = torch.randn(B, S, ns, 16, dtype=torch.float64)
    g64 = torch.randn(B, S, C * 16, dtype=torch.float64)
    if folded:
        m64 = _mlp64([8, C], False, 0.0, 5)
        f64 = torch.randn(B, S, ns, 8, dtype=torch.float64)
    else:
        m64, f64 = None, torch.randn(B, S, ns, C, dtype=torch.float64)

    def reference(dtype, device):
        f, d, w = (t.detach().to(device=device, dtype=dtype).requires_grad_(True) for t in (f64, d64, w64))
        mod = None
        z = f
        if folded:
            mod = copy.deepcopy(m64).to(device=device, dtype=dtype).train()
            mod.backend = "torch"
            z = mod(f)
        out = torch.matmul((z * d).transpose(2, 3), w).reshape(B, S, -1)
        out.backward(g64.to(device=device, dtype=dtype))
        res = {"out": out.detach(), "dfeat": f.grad, "ddens": d.grad, "dw": w.grad}
        if folded:
            res.update({n: p.grad for n, p in mod.named_parameters()})
            res.update({n: b.detach().clone() for n, b in mod.named_buffers()})
        return res

    want, t32 = reference(torch.float64, "cpu"), reference(torch.float32, dev)

    def run(o, mod):
        f, d, w = (o[n].detach().requires_grad_(True) for n in ("feat", "density", "weights"))
        if folded:
            mod.backend = "hip"; mod.train(); mod.zero_grad()
            out = feature_mlp_contract(mod, f, d, w)
        else:
            out = pointconv_contract(f, d, w)
        out.backward(o["gout"])
        res = {"out": out.detach(), "dfeat": f.grad, "ddens": d.grad, "dw": w.grad}
        if folded:
            res.update({n: p.grad.detach().clone() for n, p in mod.named_parameters()})
            res.update({n: b.detach().clone() for n, b in mod.named_buffers()})
        return res

    def check(tag, got):
        if not folded:
            for n in ("out", "dfeat", "ddens", "dw"):
                e = _err(got[n], want[n])
                assert e <= 1e-5 * max(1.0, want[n].abs().max().item()), f"{tag}: {n} {e:.3e}"
        else:                                  # everything here went through the stack: its gradient rule; running statistics by the features'
            for n in ["out", "dfeat", "ddens", "dw"] + [n for n in want if n.startswith(("weights", "gammas", "betas"))]:
                gs = max(1e-6, want[n].abs().max().item())
                e, e_t = _err(got[n], want[n]), _err(t32[n], want[n])
                assert e <= max(1e-4 * gs, 4 * e_t), f"{tag}: {n} {e:.3e} (torch fp32 {e_t:.3e}), scale {gs:.3e}"
            for n in [n for n in want if n.startswith("running")]:
                assert _err(got[n], want[n]) <= 1e-5 * max(1.0, want[n].abs().max().item()), f"{tag}: {n}"

    aligned = dict(feat=f64.float().to(dev), density=d64.float().to(dev), weights=w64.float().to(dev), gout=g64.float().to(dev))
    m32 = copy.deepcopy(m64).float().to(dev) if folded else None
    base = run(aligned, copy.deepcopy(m32))
    check("contract aligned", base)
    for k, which in enumerate(["feat", "density", "weights", "gout", "all"], start=1):
        o = dict(aligned)
        for j, key in enumerate(o):
            if which in (key, "all"):
                o[key] = _mis(shifted(o[key], (k + j) % 3 + 1))
        got = run(o, copy.deepcopy(m32))       # must not raise
        check(f"contract {which} shifted", got)
        if folded and which in ("feat", "all"):
            # (the stack's first layer stages a moved input by scalars: another kernel; printed, bounded above)
            worst = 0.0
            for n in base:
                d, sc = (got[n] - base[n]).abs().max().item(), base[n].abs().max().item()
                bound = 1e-5 * max(1.0, sc) if n.startswith("running") else 1e-4 * max(1e-6, sc)
                assert d <= bound, f"folded contraction, {which} shifted: {n} is {d:.3e} from the aligned run, bound {bound:.3e}"
                worst = max(worst, d / max(1e-30, sc))
            print(f"folded contraction, {which} shifted: largest difference to the aligned run {worst:.3e} of the tensor's max-norm")
            continue
        for n in base:
            assert torch.equal(got[n], base[n]), f"contract {which} shifted: {n} differs from the aligned run"


# ---- PointCNN's X-transform core ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,C1,C2,dm", [(8, 12, 24, 16), (12, 24, 48, 2)])
def test_xconv_core(dev, K, C1, C2, dm):
    """2 x 13 regions against the same arithmetic in fp64 under test_xconv_core_matches_fp64_composite's bound, 1e-5 * max(1, |ref|_max).  X, F1, F2, the
    taps and the bias go by scalars; the wrapper copies a misaligned upstream gradient (read as one 8- / 16-byte piece per channel): every moved
    run selects the same kernels on the same values -- bit-equal."""
    from pointcloudlib_amd.misc.pointcnn import xconv_core
    torch.manual_seed(K + C1)
    B, P, C = 2, 13, C1 + C2
    t64 = dict(X=torch.randn(B, P, K, K, dtype=torch.float64), F1=torch.randn(B, P, K, C1, dtype=torch.float64),
               F2=torch.randn(B, P, K, C2, dtype=torch.float64), wd=torch.randn(C, dm, K, dtype=torch.float64) * 0.3,
               bias=torch.randn(C * dm, dtype=torch.float64))
    gD = torch.randn(B, P, C * dm, dtype=torch.float64)
    r = {n: t.clone().requires_grad_(True) for n, t in t64.items()}
    ref = torch.einsum("bpkc,cjk->bpcj", torch.matmul(r["X"], torch.cat((r["F1"], r["F2"]), dim=-1)), r["wd"]).reshape(B, P, C * dm) + r["bias"]
    ref.backward(gD)
    want = {"D": ref.detach(), **{n: t.grad for n, t in r.items()}}

    def run(o):
        leaves = {n: o[n].detach().requires_grad_(True) for n in t64}
        out = xconv_core(leaves["X"], leaves["F1"], leaves["F2"], leaves["wd"], leaves["bias"])
        out.backward(o["gD"])
        return {"D": out.detach(), **{n: t.grad for n, t in leaves.items()}}

    aligned = {**{n: t.float().to(dev) for n, t in t64.items()}, "gD": gD.float().to(dev)}
    base = run(aligned)
    for k, which in enumerate(["aligned", "X", "F1", "F2", "wd", "bias", "gD", "all"]):
        o = dict(aligned)
        for j, key in enumerate(o):
            if which in (key, "all"):
                o[key] = _mis(shifted(o[key], (k + j) % 3 + 1))
        got = run(o)                           # must not raise
        for n, w in want.items():
            e = _err(got[n], w)
            assert e <= 1e-5 * max(1.0, w.abs().max().item()), f"xconv {which}: {n} {e:.3e}"
            assert torch.equal(got[n], base[n]), f"xconv {which} shifted: {n} differs from the aligned run"


# ---- the named exception --------------------------------------------------------------------------------------------------------------
def test_knn_point_matmul_refuses_a_misaligned_cloud(dev):
    """knn_point(form="matmul") keeps its requirement -- 16-byte aligned xyz, N a multiple of 4 -- and says so before anything is launched."""
    from pointcloudlib_amd.misc.pointconv_utils import knn_point
    xyz = torch.randn(2, 64, 3, device=dev)
    new_xyz = xyz[:, :8].contiguous()
    with pytest.raises(RuntimeError, match="16-byte aligned and N a multiple of 4"):
        knn_point(4, _mis(shifted(xyz, 1)), new_xyz, form="matmul")
    with pytest.raises(RuntimeError, match="16-byte aligned and N a multiple of 4"):
        knn_point(4, xyz[:, :63].contiguous(), new_xyz, form="matmul")


# ---- one whole step -------------------------------------------------------------------------------------------------------------------
def test_pointnet2_cls_whole_step(dev):
    """PointNet2_cls, B = 2, N = 1024, dropout off: forward + loss + backward with every parameter and buffer moved into one flat buffer at odd
    offsets (shift_module), against the aligned model under the bounds of tests/test_networks_gpu.py::test_pointnet2_cls_backends_agree_with_grads:
    logits within 1e-4 * max(1, |logits|_max), every gradient within 5e-3 of max(its max-norm, 1e-3 of the largest gradient's).

    Measured on an MI355X: the logits are bit-equal (every forward kernel is the aligned run's: the 65 536-row level keeps the resident-weight
    forward, whose buffer loads take any 4-byte alignment, the other layers change their operand staging only), the gradients differ by at
    most 7.5e-7 of their scale (the layers that leave the fused backward for dW + dX).  The comparison is a sensitive one at B = 2: the
    classifier head's BatchNorm1d normalises over two rows, and a forward that differs by 1e-6 of the features (the staged kernel in place of the
    resident-weight one at the first level) moves these logits by 1.8e-4."""
    from pointcloudlib_amd import synth
    from pointcloudlib_amd.networks.cls.pointnet2 import PointNet2_cls
    from pointcloudlib_amd.train_utils import soft_cross_entropy_loss
    torch.manual_seed(1)
    B, N = 2, 1024
    x = torch.from_numpy(synth.gauss_ball(B, N, 3)).to(dev)
    f = torch.from_numpy(synth.unit_normals(B, N, 4)).to(dev)
    lab = torch.from_numpy(synth.labels(B, 40, 3)).to(dev)
    net = PointNet2_cls().to(dev).train()
    for mod in net.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0

    def step(model):
        out = model(x, f)
        loss = soft_cross_entropy_loss(out, lab)
        loss.backward()
        return out.detach(), loss.item(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}

    moved = copy.deepcopy(net)
    where = shift_module(moved, 1)
    assert where and all(v != 0 for v in where.values()) and {4, 8, 12} <= set(where.values())
    o_a, l_a, g_a = step(copy.deepcopy(net))
    o_m, l_m, g_m = step(moved)                    # must not raise
    assert all(p.data_ptr() % 16 for p in moved.parameters())
    assert set(g_m) == set(g_a) and all(torch.isfinite(v).all() for v in g_m.values())
    missed = []
    d_o, s_o = (o_m - o_a).abs().max().item(), max(1.0, o_a.abs().max().item())
    print(f"whole step: logits differ by {d_o:.3e} (allowed {1e-4 * s_o:.3e}), loss {l_a:.6f} aligned / {l_m:.6f} moved")
    if d_o > 1e-4 * s_o:
        missed.append(f"logits {d_o:.3e} > {1e-4 * s_o:.3e}")
    gmax = max(v.abs().max().item() for v in g_a.values())
    worst = ("", 0.0)
    for n in g_a:
        s_ = max(1e-3 * gmax, g_a[n].abs().max().item())
        d = (g_m[n] - g_a[n]).abs().max().item()
        worst = max(worst, (n, d / s_), key=lambda t: t[1])
        if d > 5e-3 * s_:
            missed.append(f"grad {n} {d:.3e} > {5e-3 * s_:.3e}")
    print(f"whole step: gradients differ by at most {worst[1]:.3e} of their scale ({worst[0]}; allowed 5e-3)")
    assert not missed, missed


# ---- the narrow stacks (three layers of <= 16 channels, recomputed per pass: csrc/narrow.hip) ---------------------------------------------
def test_narrow_stack_gout(dev):
    """PointConv's WeightNet shape [3, 8, 8, 16] on 1000 rows with an input that needs no gradient: the per-stack entry point runs the narrow
    kernels, whose backward reads the upstream gradient in 16-byte pieces only where its base is 16-byte aligned.  Moved gout, x, W and vectors:
    every operand goes by scalars then (x, the parameters always), so each run is bit-equal to the aligned one; the aligned run against fp64 under
    the rule of tests/test_mlp_hip.py."""
    from pointcloudlib_amd import _lib
    spec, rows = [3, 8, 8, 16], 1000
    m64 = _mlp64(spec, True, 0.0, 21)
    x64 = torch.randn(rows, 3, dtype=torch.float64)
    g64 = torch.randn(rows, 16, dtype=torch.float64)

    def run(mod, x, g, backend):
        mod.backend = backend; mod.train(); mod.zero_grad()
        out = mod(x)                               # (x does not require grad: the narrow path's condition)
        out.backward(g)
        return (out.detach(), None, {n: p.grad.detach().clone() for n, p in mod.named_parameters()}, {n: b.detach().clone() for n, b in mod.named_buffers()})

    ref = run(copy.deepcopy(m64), x64, g64, "torch")
    m32, x32, g32 = copy.deepcopy(m64).float().to(dev), x64.float().to(dev), g64.float().to(dev)
    t32 = run(copy.deepcopy(m32), x32, g32, "torch")
    timer = _lib.KernelTimer()
    _lib.PROFILER = timer
    try:
        base = run(copy.deepcopy(m32), x32, g32, "hip")
    finally:
        _lib.PROFILER = None
    assert [n for n, _, _ in timer.order if "stack" in n] == ["pcl_mlp_stack_fwd_f32", "pcl_mlp_stack_bwd_f32"], timer.order
    zero = torch.zeros(1)
    fix = lambda r: (r[0], zero, r[2], r[3])      # noqa: E731  (no input gradient here)
    _check_mlp_fp64("narrow aligned", fix(base), fix(t32), fix(ref), True)
    for k, which in enumerate(["gout", "x", "W", "bn", "running", "all"], start=1):
        mod = copy.deepcopy(m32)
        _shift_mlp(mod, which, k)
        x = _mis(shifted(x32, k % 3 + 1)) if which in ("x", "all") else x32
        g = _mis(shifted(g32, (k + 1) % 3 + 1)) if which in ("gout", "all") else g32
        got = run(mod, x, g, "hip")                # must not raise
        _check_mlp_fp64(f"narrow {which} shifted", fix(got), fix(t32), fix(ref), True)
        _against_aligned(f"narrow {which} shifted", got, base, True)


# ---- feature propagation on packed rows (csrc/pack.hip) ----------------------------------------------------------------------------------
def test_interpolate_pack(dev):
    """ops.interpolate_pack (pcl_fp_pack_rows_f32): B = 2 clouds of 37 and 20 points (capacity 40), S = 9 sources, D2 = 6, CS = 4, two one-hot
    columns -- the widths at which the 8-byte form is chosen when points2 is 8-byte aligned.  Moved points2 (4 and 12 bytes: the one-float form;
    8 bytes: still the 8-byte form), skip, one-hot, idx3, w3: a copy and the same rounded products and sums per element either way -- rows bit-equal to the aligned run, which
    equals three_interpolate + cat on each cloud's rows (the operator's definition); gradients against the aligned run's (skip: a copy, bit-equal;
    points2: fp32 atomic adds, within 1e-6 of the gradient's max-norm -- at most 3 x 40 terms of magnitude <= |g|_max each, 2^-24 apiece)."""
    from pointcloudlib_amd.misc import ops
    B, N, S, D2, CS, n1 = 2, 40, 9, 6, 4, 2
    lengths = [37, 20]
    g = torch.Generator().manual_seed(9)
    xyz1, xyz2 = torch.randn(B, N, 3, generator=g).to(dev), torch.randn(B, S, 3, generator=g).to(dev)
    p2, sk = torch.randn(B, S, D2, generator=g).to(dev), torch.randn(B, N, CS, generator=g).to(dev)
    onehot = torch.eye(n1)[[1, 0]].to(dev)
    row_off, R = ops.row_offsets(lengths, B, N, dev)
    lens = torch.tensor(lengths, dtype=torch.int32, device=dev)
    idx3, w3 = ops.three_nn(xyz1, xyz2, lengths1=lens)
    grows = torch.randn(R, n1 + CS + D2, generator=g).to(dev)

    def run(o):
        a, b = o["points2"].detach().requires_grad_(True), o["skip"].detach().requires_grad_(True)
        rows = ops.interpolate_pack(a, o["idx3"], o["w3"], lens, row_off, R, N, skip=b, onehot=o["onehot"])
        rows.backward(grows)
        return rows.detach(), a.grad, b.grad

    aligned = dict(points2=p2, skip=sk, onehot=onehot, idx3=idx3, w3=w3)
    base = run(aligned)
    want = torch.cat([torch.cat((onehot[b].expand(lengths[b], n1), sk[b, :lengths[b]], ops.three_interpolate(p2, idx3, w3)[b, :lengths[b]]), dim=1)
                      for b in range(B)])
    assert torch.equal(base[0], want), "the aligned run differs from three_interpolate + cat"
    for which, k in [("points2", 1), ("points2", 2), ("points2", 3), ("skip", 1), ("onehot", 3), ("idx3", 1), ("w3", 2), ("all", 1)]:
        o = dict(aligned)
        for j, key in enumerate(o):
            if which in (key, "all"):
                o[key] = _mis(shifted(o[key], (k + j - 1) % 3 + 1 if which == "all" else k))
        got = run(o)                               # must not raise
        assert torch.equal(got[0], base[0]), f"interpolate_pack, {which} moved by {k}: rows differ from the aligned run"
        assert torch.equal(got[2], base[2]), f"interpolate_pack, {which} moved by {k}: the skip gradient differs"
        d = (got[1] - base[1]).abs().max().item()
        assert d <= 1e-6 * base[1].abs().max().item(), f"interpolate_pack, {which} moved by {k}: points2 gradient {d:.3e} from the aligned run"
