"""The lab switches on the host (csrc/common.h: LabSwitches; pointcloudlib_amd/_lib.py): their defaults, the environment table,
and that setting one drops what the host cached of the size queries that answer by it.  No GPU: setters, getters and size queries
are host code.  Defaults and environment are observed in child processes started fresh (the switches are process-wide)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what a child reports: every getter the header has, and the size queries that answer by a switch without one
_PROBE = """
import json
from pointcloudlib_amd import _lib
from pointcloudlib_amd.misc import mlp_hip
from pointcloudlib_amd.misc.layers import PointwiseMLP
L = _lib.lib()
m = PointwiseMLP([3, 8, 8, 16])
plan = mlp_hip._stack_plan(m, 4096, 3, 0, False, None, False, 0)
print(json.dumps(dict(
    fb_two=L.pcl_get_fb_two_images(), stack_overlap=L.pcl_get_stack_overlap(), fewrow=L.pcl_get_fewrow_backward(),
    bwd_pair=L.pcl_get_bwd_pair(), matrix_form=L.pcl_get_matrix_form(), frag_max_rows=L.pcl_frag_max_rows(),
    gather=L.pcl_group_linear_bwd_gather_supported(128), pair=L.pcl_linear_bwd_pair_supported(4096, 1024, 512, 0),
    fewrow_fused_shape=L.pcl_mlp_fewrow_layer(4096, 128, 64, 0), dw_plain_ws=L.pcl_linear_bwd_dw_plain_workspace_bytes(4096, 1024, 512),
    narrow_sizes=[plan.save_bytes, plan.fwd_tmp, plan.bwd_tmp])))
"""
_CHILDREN = {"defaults": {},
             "fewrow": {"PCL_FEWROW": "1"},
             "narrow": {"PCL_NARROW": "0"},
             "rest": {"PCL_FWD_RES": "0", "PCL_FUSED_BWD": "0", "PCL_SIDE_DW": "1", "PCL_BWD_W_ROWS": "0", "PCL_SCATTER": "0",
                      "PCL_BWD_PAIR": "0", "PCL_FB_TWO": "0", "PCL_FEWROW": "1", "PCL_DW_GX": "2"}}


@pytest.fixture(scope="module")
def children():
    """{name: what _PROBE printed} of one fresh process per entry of _CHILDREN, started together."""
    base = {k: v for k, v in os.environ.items() if not k.startswith("PCL_")}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _PROBE]
    procs = {name: subprocess.Popen(cmd, cwd=ROOT, env={**base, **env}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for name, env in _CHILDREN.items()}
    out = {}
    for name, p in procs.items():
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, (name, se[-2000:])
        out[name] = json.loads(so.splitlines()[-1])
    return out


def test_setting_a_switch_drops_the_cached_sizes():
    """A size query answered before a setter ran must not be answered from the cache after it, and a cached stack plan must be gone
    -- through the plain ``_lib.lib().pcl_set_...()`` call every caller writes, with no clearing of its own."""
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.misc import mlp_hip
    L = _lib.lib()
    try:
        assert _lib.size_query("pcl_group_linear_bwd_gather_supported", 128) == 1
        L.pcl_set_scatter_form(0)
        assert L.pcl_group_linear_bwd_gather_supported(128) == 0
        assert _lib.size_query("pcl_group_linear_bwd_gather_supported", 128) == 0
        assert _lib.size_query("pcl_linear_bwd_fused_stat_rows", 100000, 128) == 256
        L.pcl_set_fb_max_blocks(3)
        assert _lib.size_query("pcl_linear_bwd_fused_stat_rows", 100000, 128) == 3
        for name in _lib._SWITCH_SETTERS:                     # every setter of the header, with arguments that keep what is set
            args = {"pcl_set_fb_max_blocks": (3,), "pcl_set_bwd_pair": (L.pcl_get_bwd_pair(),), "pcl_set_fb_two_images": (L.pcl_get_fb_two_images(),),
                    "pcl_set_matrix_form": (0,), "pcl_set_dw_tuning": (0,), "pcl_set_fps_tuning": (0, 3),
                    "pcl_frag_set_tuning": (-1, 0, 0, 0, 0, 0, 0)}.get(name) or (-1,) * len(_lib._SIGS[name][1])
            mlp_hip._PLANS["sentinel"] = None
            getattr(L, name)(*args)
            assert "sentinel" not in mlp_hip._PLANS, name
    finally:
        mlp_hip._PLANS.pop("sentinel", None)
        L.pcl_set_scatter_form(1)
        L.pcl_set_fb_max_blocks(0)
    assert _lib.size_query("pcl_group_linear_bwd_gather_supported", 128) == 1
    assert _lib.size_query("pcl_linear_bwd_fused_stat_rows", 100000, 128) == 256
    assert len(_lib._SWITCH_SETTERS) == 12 and "pcl_frag_set_tuning" in _lib._SWITCH_SETTERS


def test_defaults_in_a_fresh_process(children):
    d = children["defaults"]
    assert (d["fb_two"], d["stack_overlap"], d["fewrow"], d["bwd_pair"], d["matrix_form"], d["frag_max_rows"]) == (1, 0, 0, 1, 0, 8192)
    assert d["gather"] == 1 and d["pair"] == 1 and d["fewrow_fused_shape"] == 0


def test_each_environment_variable_reaches_its_setter(children):
    """Through a getter, or a size query where the header has no getter.  Nothing the host can observe depends on PCL_FWD_RES
    and PCL_BWD_W_ROWS (they choose between kernels at launch only): their rows of the table are exercised -- the child that sets
    them loads and answers -- not observed."""
    d, fewrow, narrow, rest = (children[k] for k in ("defaults", "fewrow", "narrow", "rest"))
    # PCL_FEWROW alone: on, but a layer the fused dX + dW kernel has keeps it; with PCL_FUSED_BWD=0 that layer takes the few-row path
    assert fewrow["fewrow"] == 1 and fewrow["fewrow_fused_shape"] == 0
    assert rest["fewrow"] == 1 and rest["fewrow_fused_shape"] == 1
    # PCL_NARROW=0: the [3, 8, 8, 16] stack keeps its activations like any other stack
    assert narrow["narrow_sizes"] != d["narrow_sizes"] and narrow["narrow_sizes"][0] > d["narrow_sizes"][0]
    assert {k: narrow[k] for k in narrow if k != "narrow_sizes"} == {k: d[k] for k in d if k != "narrow_sizes"}
    assert rest["stack_overlap"] == 1                        # PCL_SIDE_DW
    assert rest["gather"] == 0                               # PCL_SCATTER
    assert rest["bwd_pair"] == 0 and rest["pair"] == 0       # PCL_BWD_PAIR
    assert rest["fb_two"] == 0                               # PCL_FB_TWO
    assert d["dw_plain_ws"] > rest["dw_plain_ws"] == 2 * 1024 * 512 * 4          # PCL_DW_GX=2: two row-chunk workgroups per output tile
    assert rest["matrix_form"] == 0 and rest["frag_max_rows"] == 8192            # (no variable sets these)
