"""Operands at odd storage offsets, for the alignment sweep (tests/test_operand_alignment_gpu.py).

Every tensor a test allocates is 256-byte aligned, so the half of each ``al16(...)`` predicate in csrc/ that asks about the POINTER is
never false there.  ``shifted`` puts a tensor 4, 8 or 12 bytes behind a 16-byte boundary; ``shift_module`` does it to every
parameter and buffer of a module the way a flat parameter buffer does (``p.data = flat[o:o + n].view_as(p)``)."""
import os
import re

import torch

_DTYPES = (torch.float32, torch.int32)


def shifted(t, k):
    """A copy of ``t`` whose first element lies 4*k bytes (k = 1, 2, 3) behind a 16-byte boundary: contiguous, same shape, dtype
    (float32 / int32), device, ``requires_grad`` and ``Parameter``-ness; a slice of a fresh base of ``numel + 4`` elements."""
    assert k in (1, 2, 3), f"k = {k}: 1, 2 or 3 elements"
    assert t.dtype in _DTYPES, f"shifted: float32 or int32, got {t.dtype}"
    src = t.detach()
    n = src.numel()
    base = torch.empty(n + 4, dtype=src.dtype, device=src.device)
    assert base.data_ptr() % 16 == 0, "a fresh allocation is expected to be 16-byte aligned"
    view = base[k:k + n].view(src.shape)
    view.copy_(src)
    if isinstance(t, torch.nn.Parameter):
        out = torch.nn.Parameter(view, requires_grad=t.requires_grad)
    else:
        out = view.requires_grad_(t.requires_grad)
    assert out.data_ptr() % 16 == 4 * k and out.is_contiguous() and out.shape == t.shape
    return out


def shift_module(module, k):
    """Re-point every float32 / int32 parameter and buffer of ``module`` at a slice of ONE flat buffer per (dtype, device), each with
    an odd-sized gap in front: tensor i starts ((k - 1 + i) % 3 + 1) elements behind a 16-byte boundary, so none is aligned and all
    three residues occur.  The Parameter / buffer objects stay (only ``.data`` moves), values are kept, gradients are dropped.
    Returns {name: data_ptr % 16}."""
    assert k in (1, 2, 3)
    named = [(n, p) for n, p in module.named_parameters()] + [(n, b) for n, b in module.named_buffers()]
    named = [(n, t) for n, t in named if t.dtype in _DTYPES and t.numel() > 0]
    groups = {}
    for n, t in named:
        groups.setdefault((t.dtype, t.device), []).append((n, t))
    where = {}
    for (dtype, device), items in groups.items():
        offs, o = [], 0
        for i, (_, t) in enumerate(items):
            want = (k - 1 + i) % 3 + 1
            o += 1                                   # (a gap of at least one element: no two tensors touch)
            while o % 4 != want:
                o += 1
            offs.append(o)
            o += t.numel()
        flat = torch.empty(o + 4, dtype=dtype, device=device)
        assert flat.data_ptr() % 16 == 0
        for (n, t), off in zip(items, offs):
            piece = flat[off:off + t.numel()].view(t.shape)
            piece.copy_(t.detach())
            t.data = piece
            if isinstance(t, torch.nn.Parameter):
                t.grad = None
            assert t.data_ptr() % 16 == 4 * (off % 4) != 0 and t.is_contiguous()
            where[n] = t.data_ptr() % 16
    return where


# ---- the scan behind the inventory test: which functions of csrc/*.hip ask about a pointer's alignment ------------------------------
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pointcloudlib_amd", "csrc")
_HEAD = re.compile(r"^(?!namespace|using|struct|constexpr|typedef|template|#|//|/\*|\}|\{)[A-Za-z_][^;{}]*?\b([A-Za-z_]\w*)\s*\(")
_ATTR = re.compile(r"__launch_bounds__\([^)]*\)|__attribute__\(\([^)]*\)\)")
# a call of al16(...) (common.h) or aligned8(...) (pack.hip), or a hand-written test of a pointer's low bits
_ASKS = re.compile(r"\bal16\(|\baligned8\(|uintptr_t.*&\s*(15|7)\b")


def al16_functions(csrc=CSRC):
    """{(file, function)} for every function definition of ``csrc/*.hip`` (host or device) whose body asks about the alignment of a
    pointer: ``al16(``, ``aligned8(`` or a mask of a ``uintptr_t`` with 15 / 7.  Definitions start in column 0 in this code base (also
    inside ``namespace pcl``); the name is the identifier in front of the first ``(`` of that line, attributes aside."""
    found = set()
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith(".hip"):
            continue
        cur = None
        with open(os.path.join(csrc, fn)) as f:
            for line in f:
                code = line.split("//")[0]
                m = _HEAD.match(_ATTR.sub("", code))
                if m and not code.rstrip().endswith(";"):
                    cur = m.group(1)
                if _ASKS.search(code):
                    assert cur is not None, f"{fn}: an alignment question outside a function: {line!r}"
                    found.add((fn, cur))
    return found
