"""CPU: planning of the opt-in one-launch attention backward for wide key windows (attn_bwd6_kernel, plan name ``bwd6``): with the
switch off every plan is the default one; with it on, bwd6 exactly where its admission rule says and the default plan everywhere
else; the setter wins over the environment."""
import os
import subprocess
import sys

import pytest
import torch

from tests.test_planning_cpu import _attn_geoms
from xpretrain_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FG, R_MAX = 208, 1152          # rows of one LDS group (attn_bwd5's limit); rows attn_bwd6's LDS constant arrays hold
CUS = (256, 80, 36, 8)
REGIONS = ("part", "delta", "dq", "dkv", "counter")


def _plans(mode, B, H, S, M, N, Lp):
    """every (f32, pad, cus, bwd) plan of a geometry, keyed by those arguments"""
    from xpretrain_amd import hip_ops as Hh
    size = (M, N, Lp) if mode == L.ATTN_PROXY else None
    return {(f32, pad, cus, bwd): Hh.attn_plan(B, S, H, size=size, pad_mask=(True if pad else None),
                                               dtype=(torch.float32 if f32 else torch.bfloat16), backward=bwd, cus=cus)
            for f32 in (False, True) for pad in (False, True) for cus in CUS for bwd in (False, True)}


def _wide_geoms():
    """the yardstick's geometries plus R = M + L on both sides of 208 and of R_MAX, with M on both sides of 16"""
    yield from _attn_geoms()
    for B, H in ((1, 2), (8, 12)):
        for M, Lp in ((4, 204), (4, 205), (16, 192), (16, 193), (4, R_MAX - 4), (4, R_MAX - 3), (16, R_MAX - 16), (16, R_MAX - 15),
                      (17, 400), (1, 2000)):
            for N in (1, 8):
                yield L.ATTN_PROXY, B, H, M + N * Lp, M, N, Lp


@pytest.fixture
def switch(monkeypatch):
    """the library's switch, restored after the test; XPRETRAIN_DEBUG unset"""
    lib = L.lib()
    prev = lib.xp_get_attn_bwd_wide()
    monkeypatch.delenv("XPRETRAIN_DEBUG", raising=False)
    try:
        yield lib
    finally:
        lib.xp_set_attn_bwd_wide(prev)


def test_switch_off_plans_are_the_default_plans():
    """environment unset, setter never called (a fresh interpreter) against this process with the setter at 0: every field of every
    plan of the yardstick's geometries is equal"""
    code = ("import json, sys; sys.path.insert(0, %r)\n"
            "from tests.test_attention_wide_bwd_planning_cpu import _plans\n"
            "from tests.test_planning_cpu import _attn_geoms\n"
            "print(json.dumps([sorted((repr(k), v) for k, v in _plans(*g).items()) for g in _attn_geoms()]))" % ROOT)
    env = {k: v for k, v in os.environ.items() if k not in ("XPRETRAIN_ATTN_BWD_WIDE", "XPRETRAIN_DEBUG")}
    untouched = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, check=True, capture_output=True, text=True).stdout
    import json
    untouched = json.loads(untouched.strip().splitlines()[-1])
    lib = L.lib()
    prev = lib.xp_get_attn_bwd_wide()
    saved = os.environ.pop("XPRETRAIN_DEBUG", None)
    try:
        assert lib.xp_set_attn_bwd_wide(0) == 0 and lib.xp_get_attn_bwd_wide() == 0
        for g, want in zip(_attn_geoms(), untouched):
            got = json.loads(json.dumps(sorted((repr(k), v) for k, v in _plans(*g).items())))
            assert len(got) == len(want)
            for (ka, a), (kb, b) in zip(got, want):
                assert ka == kb and a.keys() == b.keys()
                for f in a:
                    assert a[f] == b[f], (g, ka, f, a[f], b[f])
                assert a["kernel"] != "bwd6"
    finally:
        lib.xp_set_attn_bwd_wide(prev)
        if saved is not None:
            os.environ["XPRETRAIN_DEBUG"] = saved


@pytest.mark.parametrize("split", [False, True])
def test_switch_on_plans_bwd6_exactly_where_admitted(split, switch, monkeypatch):
    """bwd6: backward, bf16, PROXY, M <= 16, no padding mask, 208 < R <= R_MAX, XPRETRAIN_DEBUG=attn_bwd_split not set; there the grid
    is min(problems, CUs), dynamic LDS fits a CU, the problem counter is used, the workspace regions are the default plan's (disjoint,
    inside the unchanged xp_attn_workspace_bytes) and the column-sum rows are xp_attn_bwd_colsum_rows.  Everywhere else -- fp32,
    causal, forward, a padding mask, M > 16, R outside the range, the split flag -- the plan is the default one, field by field."""
    lib = switch
    seen = {"bwd6": 0, "low": 0, "high": 0, "m17": 0, "pad": 0, "f32": 0, "causal": 0, "fwd": 0}
    for geom in _wide_geoms():
        mode, B, Hh, S, M, N, Lp = geom
        monkeypatch.delenv("XPRETRAIN_DEBUG", raising=False)
        lib.xp_set_attn_bwd_wide(0)
        default = _plans(*geom)
        ws_off = lib.xp_attn_workspace_bytes(mode, B, Hh, M, N, Lp)
        lib.xp_set_attn_bwd_wide(1)
        if split:
            monkeypatch.setenv("XPRETRAIN_DEBUG", "attn_bwd_split")
            lib.xp_set_attn_bwd_wide(0)
            default_split = _plans(*geom)
            lib.xp_set_attn_bwd_wide(1)
        on = _plans(*geom)
        ws = lib.xp_attn_workspace_bytes(mode, B, Hh, M, N, Lp)
        assert ws == ws_off == (4 * max(B * Hh * N * M * 66, B * Hh * S + B * Hh * N * M * 192 + 64) if mode == L.ATTN_PROXY else 4 * B * Hh * S)
        R, P = (M + Lp if mode == L.ATTN_PROXY else S), B * Hh * N
        for (f32, pad, cus, bwd), p in on.items():
            case = (geom, f32, pad, cus, bwd, p)
            admitted = bwd and not f32 and mode == L.ATTN_PROXY and M <= 16 and not pad and FG < R <= R_MAX and not split
            assert (p["kernel"] == "bwd6") == admitted, case
            if not admitted:
                assert p == (default_split if split else default)[(f32, pad, cus, bwd)], case
                for name, hit in (("low", R <= FG), ("high", R > R_MAX), ("m17", M > 16), ("pad", pad), ("f32", f32),
                                  ("causal", mode == L.ATTN_CAUSAL), ("fwd", not bwd)):
                    seen[name] += bool(hit)
                continue
            seen["bwd6"] += 1
            d = default[(f32, pad, cus, bwd)]
            assert d["kernel"] == "bwd_pair", case
            assert p["grid"] == min(P, cus) and 0 < p["lds_bytes"] <= 160 * 1024 and p["uses_counter"] == 1, case
            assert p["reduce_grid"] == d["reduce_grid"] == B * Hh * M, case
            assert all(p[r] == d[r] for r in REGIONS) and p["workspace_bytes"] == d["workspace_bytes"], case
            assert p["counter"][1] >= 4 and p["part"][1] == 0, case
            used = sorted(p[r] for r in REGIONS if p[r][1])
            assert all(a[0] + a[1] <= b[0] for a, b in zip(used, used[1:])), case
            assert used[-1][0] + used[-1][1] == p["workspace_bytes"] <= ws, case
            assert p["colsum_rows"] == lib.xp_attn_bwd_colsum_rows(mode, B, Hh, S, M, N, Lp, L.XP_BF16) > 0, case
    assert (seen["bwd6"] > 0) == (not split) and all(v > 0 for k, v in seen.items() if k != "bwd6"), seen


def test_widest_tested_window_is_admitted(switch):
    """M = 16 with L = 1023 (the widest window the attention tests run) is inside R_MAX"""
    from xpretrain_amd import hip_ops as Hh
    switch.xp_set_attn_bwd_wide(1)
    assert Hh.attn_plan(1, 16 + 2 * 1023, 1, size=(16, 2, 1023), backward=True, cus=256)["kernel"] == "bwd6"
    assert Hh.attn_plan(8, 4 + 8 * 784, 12, size=(4, 8, 784), backward=True, cus=256)["grid"] == 256


def test_setter_wins_over_the_environment(switch):
    """XPRETRAIN_ATTN_BWD_WIDE gives the initial value (unset, empty, 0: off); xp_set_attn_bwd_wide overrides it either way;
    xp_get_attn_bwd_wide reads the state back; the Python wrappers go through the same state"""
    from xpretrain_amd import hip_ops as Hh
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from xpretrain_amd import _lib as L, hip_ops as H\n"
            "lib = L.lib()\n"
            "k = lambda: H.attn_plan(2, 4 + 3 * 300, 2, size=(4, 3, 300), backward=True, cus=256)['kernel']\n"
            "out = [lib.xp_get_attn_bwd_wide(), k()]\n"
            "for v in (0, 1, 0, 5):\n"
            "    assert lib.xp_set_attn_bwd_wide(v) == 0\n"
            "    out += [lib.xp_get_attn_bwd_wide(), k()]\n"
            "print(out)" % ROOT)
    for val, first in ((None, [0, "bwd_pair"]), ("", [0, "bwd_pair"]), ("0", [0, "bwd_pair"]), ("1", [1, "bwd6"])):
        env = {k: v for k, v in os.environ.items() if k not in ("XPRETRAIN_ATTN_BWD_WIDE", "XPRETRAIN_DEBUG")}
        if val is not None:
            env["XPRETRAIN_ATTN_BWD_WIDE"] = val
        got = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, check=True, capture_output=True, text=True).stdout
        assert eval(got.strip().splitlines()[-1]) == first + [0, "bwd_pair", 1, "bwd6", 0, "bwd_pair", 1, "bwd6"], (val, got)
    Hh.set_attn_bwd_wide(True)
    assert Hh.get_attn_bwd_wide() is True and switch.xp_get_attn_bwd_wide() == 1
    Hh.set_attn_bwd_wide(False)
    assert Hh.get_attn_bwd_wide() is False and switch.xp_get_attn_bwd_wide() == 0
