"""Host-only checks of the regenerating backward of the folded first layer: where Uf lives, and argument validation."""
import ctypes


def _al256(n):
    return (n + 255) // 256 * 256


def _wide_desc(B, N, m, ns, Cf, spec):
    from pointcloudlib_amd import _lib
    S = _lib.struct("pcl_mlp_stack_t")
    d = S()
    d.struct_bytes = ctypes.sizeof(S)
    d.n_layers = len(spec)
    d.c[0] = 3 + Cf
    for l, c in enumerate(spec):
        d.c[l + 1] = c
    d.P, d.pool, d.grouped, d.need_dx = B * m * ns, ns, 1, 1
    d.B, d.N, d.m, d.Cf, d.use_xyz = B, N, m, Cf, 1
    d.slope, d.out_slope, d.eps, d.momentum = 0.0, 0.0, 1e-5, 0.1
    d.xyz = d.new_xyz = d.idx = d.cnt = d.group_off = 1          # (non-null is all the size query wants)
    d.feature = d.Wf_dense = 1
    for l in range(len(spec)):
        d.layer[l].W = d.layer[l].gamma = d.layer[l].beta = 1
    return d


def _sizes(d):
    from pointcloudlib_amd import _lib
    sv, ft, bt = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    assert _lib.lib().pcl_mlp_stack_sizes(ctypes.byref(d), ctypes.byref(sv), ctypes.byref(ft), ctypes.byref(bt)) == 0
    return sv.value, ft.value


def test_uf_moves_from_the_forward_scratch_to_the_saved_buffer():
    """Grouped stack with wide features (the second level of PointNet++ SSG): the backward forms y from Uf, so Uf [B*N, c1] lives in `save`
    and no longer in the forward's `tmp`: save + fwd_tmp is what it was.  With the scatter form switched to atomics the backward reads Y
    and Uf stays in `tmp`; the difference between the two layouts is then exactly Uf and the two row lists of the gather."""
    from pointcloudlib_amd import _lib
    L = _lib.lib()
    B, N, m, ns, Cf, spec = 32, 512, 128, 64, 128, [128, 128, 256]
    d = _wide_desc(B, N, m, ns, Cf, spec)
    uf = _al256(B * N * spec[0] * 4)
    lists = _al256((B * N + 1) * 4) + _al256(B * m * ns * 4)
    assert uf == 8 * 1024 * 1024
    try:
        assert L.pcl_group_linear_bwd_gather_supported(spec[0]) == 1
        sv, ft = _sizes(d)
        L.pcl_set_scatter_form(0)
        sv0, ft0 = _sizes(d)
    finally:
        L.pcl_set_scatter_form(1)
    assert sv - sv0 == lists + uf
    assert ft0 - ft == uf
    assert sv + ft == sv0 + ft0 + lists


def test_regen_entry_points_validate_on_the_host():
    from pointcloudlib_amd import _lib
    L = _lib.lib()
    assert [L.pcl_group_linear_bwd_regen_supported(c, f) for c, f in ((64, 0), (128, 3), (256, 4), (96, 3), (64, 5), (512, 0))] == [1, 1, 1, 0, 0, 0]
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf) // 16 * 16 + 16)
    q = ctypes.c_void_p(p.value + 4)
    assert L.pcl_group_linear_bwd_regen_f32(p, p, p, p, 3, 6, p, p, p, p, p, p, 96, p, p, None, 0, 0, None) == -1            # C1 = 96
    assert b"C1" in L.pcl_last_error()
    assert L.pcl_group_linear_bwd_regen_f32(p, None, None, None, 0, 0, p, p, p, p, p, p, 64, p, None, None, 0, 0, None) == -1   # no weights
    assert L.pcl_group_linear_bwd_regen_f32(p, p, p, p, 3, 6, q, p, p, p, p, p, 64, p, p, None, 0, 0, None) == -1            # dU not 16-byte aligned
    assert b"aligned" in L.pcl_last_error()
    assert L.pcl_group_linear_bwd_gather_regen_f32(p, p, None, p, 3, p, p, p, p, p, p, 1, 8, 128, p, None, None, 0, None) == -1     # no Uf
    assert b"null" in L.pcl_last_error()
    assert L.pcl_group_linear_bwd_gather_regen_f32(p, p, p, p, 3, p, p, p, p, p, p, 1, 8, 96, p, None, None, 0, None) == -1        # C1 = 96
