"""CPU: the helpers of the alignment sweep (tests/misaligned.py) and the inventory of the alignment-dependent dispatches
(INVENTORY in tests/test_operand_alignment_gpu.py, the table of DESIGN.md section 22) against the source."""
import copy
import os

import pytest
import torch
from torch import nn

from misaligned import CSRC, al16_functions, shift_module, shifted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
def test_shifted_moves_a_tensor_off_the_16_byte_grid(k, dtype):
    t = (torch.arange(35).reshape(5, 7) * 3 - 20).to(dtype)
    s = shifted(t, k)
    assert s.data_ptr() % 16 == 4 * k and s.is_contiguous() and s.dtype == dtype and s.shape == t.shape
    assert torch.equal(s, t) and s.data_ptr() != t.data_ptr() and not s.requires_grad
    assert s.untyped_storage().nbytes() == 4 * (t.numel() + 4)              # a slice of a base of numel + 4 elements
    v = shifted(t.t(), k)                                                   # a non-contiguous source: same values, dense result
    assert torch.equal(v, t.t()) and v.is_contiguous() and v.data_ptr() % 16 == 4 * k


def test_shifted_keeps_requires_grad_and_parameters():
    t = torch.randn(3, 4, requires_grad=True)
    s = shifted(t, 2)
    assert s.requires_grad and s.is_leaf and not isinstance(s, nn.Parameter)
    (s * 2).sum().backward()
    assert torch.equal(s.grad, torch.full((3, 4), 2.0)) and t.grad is None
    p = shifted(nn.Parameter(torch.randn(6)), 3)
    assert isinstance(p, nn.Parameter) and p.requires_grad and p.data_ptr() % 16 == 12
    q = shifted(nn.Parameter(torch.randn(6), requires_grad=False), 1)
    assert isinstance(q, nn.Parameter) and not q.requires_grad
    with pytest.raises(AssertionError):
        shifted(torch.zeros(4, dtype=torch.float64), 1)
    with pytest.raises(AssertionError):
        shifted(torch.zeros(4), 0)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_shift_module_moves_every_parameter_and_buffer_into_one_flat_buffer(k):
    torch.manual_seed(k)
    net = nn.Sequential(nn.Linear(9, 40), nn.BatchNorm1d(40), nn.ReLU(), nn.Linear(40, 50, bias=True), nn.BatchNorm1d(50), nn.Linear(50, 3))
    net[1].running_mean.normal_(); net[4].running_var.uniform_(0.5, 2.0)
    ref = copy.deepcopy(net)
    params, bufs = list(net.parameters()), list(net.buffers())
    where = shift_module(net, k)
    assert [id(p) for p in net.parameters()] == [id(p) for p in params] and [id(b) for b in net.buffers()] == [id(b) for b in bufs]
    floats = [n for n, t in list(ref.named_parameters()) + list(ref.named_buffers()) if t.dtype == torch.float32]
    assert sorted(where) == sorted(floats) and set(where.values()) == {4, 8, 12}
    assert all(t.data_ptr() % 16 == where[n] for n, t in list(net.named_parameters()) + list(net.named_buffers()) if n in where)
    stores = {t.untyped_storage().data_ptr() for n, t in list(net.named_parameters()) + list(net.named_buffers()) if n in where}
    assert len(stores) == 1, "one flat buffer"
    spans = sorted((t.data_ptr(), t.data_ptr() + 4 * t.numel()) for n, t in list(net.named_parameters()) + list(net.named_buffers()) if n in where)
    assert all(a[1] < b[0] for a, b in zip(spans, spans[1:])), "a gap in front of every tensor"
    assert net[1].num_batches_tracked.dtype == torch.int64                  # (not a kernel operand: left where it is)
    for (n, a), (_, b) in zip(net.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), n
    x = torch.randn(7, 9)
    ya, yb = net(x), ref(x)
    assert torch.equal(ya, yb)
    ya.square().sum().backward(); yb.square().sum().backward()
    for (n, a), (_, b) in zip(net.named_parameters(), ref.named_parameters()):
        assert torch.equal(a.grad, b.grad), n
    with torch.no_grad():                                                   # an in-place update lands in the flat buffer
        for p in net.parameters():
            p.add_(1.0)
    assert torch.equal(net[0].weight, ref[0].weight + 1.0)


def test_every_function_that_asks_al16_is_in_the_inventory():
    """The sweep cannot go stale: a new alignment question in csrc/*.hip (``al16(``, ``aligned8(``, a mask of a pointer's low bits, host or
    device) -- a new alignment-dependent dispatch -- fails here until it has a row
    (and a covering case) in INVENTORY and in DESIGN.md."""
    from test_operand_alignment_gpu import INVENTORY
    found = al16_functions()
    assert len(found) >= 30, f"the scan found {len(found)} functions only: did csrc move? ({CSRC})"
    missing, stale = sorted(found - set(INVENTORY)), sorted(set(INVENTORY) - found)
    assert not missing, f"functions of csrc/*.hip that ask al16(...) without a row in INVENTORY: {missing}"
    assert not stale, f"INVENTORY rows whose function no longer asks al16(...): {stale}"
    import test_operand_alignment_gpu as sweep
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for (fn, func), row in INVENTORY.items():
        assert set(row) == {"entry", "external", "misaligned", "case"}, (fn, func)
        assert row["entry"] and row["external"] and row["misaligned"] and row["case"], (fn, func)
        assert row["misaligned"].startswith(("kernel", "error")), (fn, func, row["misaligned"])
        for name in row["case"].replace("/", " ").replace("(", " ").split():
            if name.startswith("test_") and "::" not in name and ".py" not in name:
                assert hasattr(sweep, name), f"{func}: covering case {name} does not exist"
        assert f"`{func}`" in design, f"DESIGN.md section 22 has no row for {func} ({fn})"


def test_the_scan_finds_a_function_by_its_definition_line(tmp_path):
    (tmp_path / "a.hip").write_text(
        'namespace pcl {\nstatic bool wide(int K, const float* X) {\n    return K % 4 == 0 && al16(X);\n}\n'
        '// al16(in a comment) does not count\ntemplate <int A>\nstatic int launch_t(const Args& a,\n        hipStream_t st) {\n'
        '    const bool vec = al16(a.A, a.B);\n    return 0;\n}\n}\nextern "C" int pcl_entry_f32(const float* x) {\n'
        '    PCL_REQUIRE(al16(x), "aligned");\n    return helper(x);\n}\nint pcl::impl(const float* y) { return al16(y) ? 1 : 0; }\n')
    (tmp_path / "b.h").write_text("inline bool al16(const void* p) { return true; }\n")
    (tmp_path / "c.hip").write_text(
        'template <int L>\n__global__ __launch_bounds__(256) void k_bwd(const float* g) {\n'
        '    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) { }\n}\nstatic inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }\n'
        'extern "C" int pcl_pack(const float* p2) {\n    const bool vec = aligned8(p2);\n    return vec;\n}\n')
    assert al16_functions(str(tmp_path)) == {("a.hip", "wide"), ("a.hip", "launch_t"), ("a.hip", "pcl_entry_f32"), ("a.hip", "impl"),
                                             ("c.hip", "k_bwd"), ("c.hip", "aligned8"), ("c.hip", "pcl_pack")}
