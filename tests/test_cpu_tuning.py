"""The switch table (roma_amd/csrc/tuning.hip) seen through roma_tuning / roma_tuning_describe: no GPU needed.

The expected inventory below is a copy of what the sources held BEFORE the table existed (the `if` chain of roma_tuning in
api.hip and the hand-written getenv lines of fifteen files): it is frozen here on purpose and not derived from the table."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

from conftest import ROOT

CSRC = os.path.join(ROOT, "roma_amd", "csrc")

# roma_tuning key -> (environment variable or None, default)
KEYS = {
    "gemm8p": ("ROMA_GEMM8P", 1), "gemm_dbg": ("ROMA_GEMM_DBG", 0), "gemm8p_walk": (None, -1),
    "gemm8p_sched": ("ROMA_GEMM8P_SCHED", 1), "gemm8p_maxwg": (None, -1), "ws1x1": ("ROMA_WS1X1", 1),
    "lc_mode": ("ROMA_LC_MODE", 0), "lc_bin": ("ROMA_LC_BIN", 1), "conv64": ("ROMA_CONV64", 7),
    "conv_patch": ("ROMA_CONV_PATCH", 1), "attn_xcd": ("ROMA_ATTN_XCD", 1), "attn_exp2": (None, -1),
    "dw_ring": ("ROMA_DW_RING", 1), "gp_col": ("ROMA_GP_COL", 1), "pool_proj": ("ROMA_POOL_PROJ", 1),
    "gp_col_leader": ("ROMA_GP_COL_LEADER", 1),
}
# environment variables without a key -> default
ENV_ONLY = {
    "ROMA_GEMM8P_MINM": 2048, "ROMA_GEMM_NT": 1, "ROMA_GEMM_F32_FILL": 1, "ROMA_GEMM_SMALLM": 1, "ROMA_CONV64_SY": 0,
    "ROMA_CONV_KORDER": 1, "ROMA_RB_SY": 0,
    "ROMA_DWR_MAXSY": 1 << 20, "ROMA_DW_RING_MINELEMS": 64 << 20, "ROMA_RI_VEC": 1, "ROMA_OUT_ROW": 1, "ROMA_OUT_LPR": 1,
    "ROMA_OUT_ROWS_IT": 0, "ROMA_GP_AUG": 1, "ROMA_GP_BWD2": 1, "ROMA_COMPOSE_OUT": 1, "ROMA_VIT_RES_F32": 0,
    "ROMA_STREAMS": 0, "ROMA_STREAMS_SERIAL": 0, "ROMA_DEBUG_DUAL_SLOT": -1,
}
# the switches of the refiner-block variants that were removed (the C = 576 one-kernel block, the two-barrier workgroup kernel):
# (key, environment variable) of their six rows, frozen - none may come back as a key or an environment name
RETIRED = (("rb24w", "ROMA_RB24W"), ("rb144_1b", "ROMA_RB144_1B"), ("rb_wide", "ROMA_RB_WIDE"), (None, "ROMA_RB_DBG"),
           (None, "ROMA_RB_WIDE_PK"), (None, "ROMA_RBW_DBG"))
ENV_DEFAULTS = {**{e: d for e, d in KEYS.values() if e}, **ENV_ONLY}
# the globals the keys used to live in
FORMER_GLOBALS = ["g_gemm_tuning", "g_gemm8p_walk", "g_gemm8p_sched", "g_gemm8p_maxwg", "g_ws1x1_mode", "g_lc_mode", "g_lc_bin",
                  "g_conv64_mode", "g_conv_patch", "g_attn_xcd_map", "g_attn_exp2", "g_rb24_wave", "g_rb144_1b", "g_rb_wide",
                  "g_dw_ring", "g_gp_col", "g_pool_proj", "g_gp_col_leader"]


def describe(lib):
    n = lib.roma_tuning_describe(None, 0)
    buf = C.create_string_buffer(int(n))
    assert lib.roma_tuning_describe(buf, n) == n and lib.roma_tuning_describe(buf, n - 1) < 0
    return json.loads(buf.value.decode())


def test_inventory_is_the_frozen_one_in_both_libraries(built_lib):
    from roma_amd import _lib
    assert len(KEYS) == 16 and len(ENV_DEFAULTS) == 33
    per_lib = []
    for fmt in ("bf16", "f16"):
        rows = describe(_lib.load(fmt))
        assert sorted(r["key"] for r in rows if r["key"]) == sorted(KEYS), fmt
        assert sorted(r["env"] for r in rows if r["env"]) == sorted(ENV_DEFAULTS), fmt
        for r in rows:
            assert r["key"] or r["env"], r
            if r["key"]:
                assert (r["env"], r["default"]) == KEYS[r["key"]], r
            else:
                assert r["default"] == ENV_ONLY[r["env"]], r
            assert r["doc"], r
        per_lib.append([(r["key"], r["env"], r["default"], r["doc"]) for r in rows])
    assert per_lib[0] == per_lib[1]


def test_retired_switches_are_gone_from_both_libraries(built_lib):
    from roma_amd import _lib
    retired = {n for row in RETIRED for n in row if n}
    assert len(RETIRED) == 6 and len(retired) == 9 and not retired & (set(KEYS) | set(ENV_DEFAULTS))
    for fmt in ("bf16", "f16"):
        lib = _lib.load(fmt)
        rows = describe(lib)
        assert set(rows[0]) == {"key", "env", "default", "override", "value", "doc"}
        names = {r["key"] for r in rows} | {r["env"] for r in rows}
        assert not names & retired, (fmt, names & retired)
        for key in [k for k, _ in RETIRED if k]:
            assert lib.roma_tuning(key.encode(), 1) == -1, (fmt, key)  # ROMA_ERR_ARG
            assert lib.roma_last_error().decode() == "roma_tuning: unknown key " + key


CHILD = r"""
import ctypes as C, json, sys
def load(path):
    lib = C.CDLL(path)
    lib.roma_tuning_describe.restype = C.c_long
    lib.roma_tuning_describe.argtypes = [C.c_char_p, C.c_long]
    lib.roma_tuning.argtypes = [C.c_char_p, C.c_int]
    lib.roma_last_error.restype = C.c_char_p
    return lib
def describe(lib):
    n = lib.roma_tuning_describe(None, 0)
    buf = C.create_string_buffer(n)
    assert lib.roma_tuning_describe(buf, n) == n
    return json.loads(buf.value.decode())
a, b = load(sys.argv[1]), load(sys.argv[2])
keys = [r["key"] for r in describe(a) if r["key"]]
out = {"env_a": describe(a), "env_b": describe(b)}
out["set_rc"] = [a.roma_tuning(k.encode(), 11) for k in keys]
out["set_a"], out["other_b"] = describe(a), describe(b)
out["clear_rc"] = [a.roma_tuning(k.encode(), -1) for k in keys]
out["clear_a"] = describe(a)
floors = {}
for k, v in (("gemm8p_walk", 0), ("gemm8p_walk", 1), ("gemm8p_maxwg", 7), ("gemm8p_maxwg", 8), ("gemm8p", 0)):
    assert a.roma_tuning(k.encode(), v) == 0
    floors["%s=%d" % (k, v)] = [r for r in describe(a) if r["key"] == k][0]
    assert a.roma_tuning(k.encode(), -1) == 0
out["floors"] = floors
assert b.roma_tuning(b"lc_bin", 0) == 0
out["b_set_a"], out["b_set_b"] = describe(a), describe(b)
out["unknown_rc"] = a.roma_tuning(b"no_such_switch", 1)
out["unknown_err"] = a.roma_last_error().decode()
print(json.dumps(out))
"""


def test_environment_override_and_clear_in_a_fresh_process(built_lib):
    from roma_amd import _lib
    env = dict(os.environ)
    env_set = {e: d + 3 for e, d in ENV_DEFAULTS.items()}
    env_set["ROMA_DW_RING_MINELEMS"] = 5_000_000_000  # values are long, not int
    env.update({e: str(v) for e, v in env_set.items()})
    run = subprocess.run([sys.executable, "-c", CHILD, _lib.LIB_PATHS["bf16"], _lib.LIB_PATHS["f16"]], capture_output=True, text=True,
                         timeout=120, env=env)
    assert run.returncode == 0, run.stderr
    out = json.loads(run.stdout)

    def env_value(r):  # what the row resolves to with no override
        return r["default"] if r["env"] is None else env_set[r["env"]]

    # the environment is honoured, by both libraries
    for rows in (out["env_a"], out["env_b"]):
        for r in rows:
            assert r["override"] is None and r["value"] == env_value(r), r
    # an override beats it; -1 brings it back
    assert out["set_rc"] == [0] * 16 and out["clear_rc"] == [0] * 16
    for r in out["set_a"]:
        assert (r["override"], r["value"]) == ((11, 11) if r["key"] else (None, env_value(r))), r
    assert out["clear_a"] == out["env_a"]
    # the two keys with a higher floor
    f = out["floors"]
    assert (f["gemm8p_walk=0"]["override"], f["gemm8p_walk=0"]["value"]) == (None, -1)
    assert (f["gemm8p_walk=1"]["override"], f["gemm8p_walk=1"]["value"]) == (1, 1)
    assert (f["gemm8p_maxwg=7"]["override"], f["gemm8p_maxwg=7"]["value"]) == (None, -1)
    assert (f["gemm8p_maxwg=8"]["override"], f["gemm8p_maxwg=8"]["value"]) == (8, 8)
    assert (f["gemm8p=0"]["override"], f["gemm8p=0"]["value"]) == (0, 0)
    # each library owns its table
    assert out["other_b"] == out["env_b"]
    assert out["b_set_a"] == out["env_a"]
    changed = [r["key"] for r, r0 in zip(out["b_set_b"], out["env_b"]) if r != r0]
    assert changed == ["lc_bin"]
    # unknown key
    assert out["unknown_rc"] == -1 and out["unknown_err"] == "roma_tuning: unknown key no_such_switch"


def test_unknown_key_in_process(built_lib):
    assert built_lib.roma_tuning(b"no_such_switch", 1) == -1  # ROMA_ERR_ARG
    assert b"no_such_switch" in built_lib.roma_last_error()
    assert built_lib.roma_tuning(None, 1) == -1 and b"null key" in built_lib.roma_last_error()


def test_switches_live_in_the_table_only():
    getenv_sites, extern_sites = [], []
    former = re.compile(r"\bint\s+(%s)\b" % "|".join(FORMER_GLOBALS))  # declaration or definition
    for name in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, name)
        if not os.path.isfile(path) or name.endswith((".o", ".d")):
            continue
        with open(path, errors="replace") as f:
            for i, line in enumerate(f, 1):
                if 'getenv("ROMA_' in line:
                    getenv_sites.append((name, line.strip()))
                if former.search(line):
                    extern_sites.append((name, i))
    assert extern_sites == []
    # the table builds its names from the rows, so the one literal read left is the comma-separated ROMA_DEBUG_ONLY
    assert [n for n, _ in getenv_sites] == ["model.hip"], getenv_sites
    assert getenv_sites[0][1].count('getenv("ROMA_') == getenv_sites[0][1].count('getenv("ROMA_DEBUG_ONLY")') == 2


def test_integration_md_lists_every_switch(built_lib):
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for r in describe(built_lib):
        for name in (r["key"], r["env"]):
            assert name is None or "`%s`" % name in doc, name
