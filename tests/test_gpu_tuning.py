"""The environment half of the switch table (roma_amd/csrc/tuning.hip) on a real launch: ROMA_GEMM8P=0 keeps a GEMM off the
8-phase kernel, roma_tuning("gemm8p", 1) beats the environment, and the kernels agree bit for bit.  The environment is read
once per process, so each case is a fresh child."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

# bf16 GEMM M = 8192, N = 256, K = 256: the smallest shape gemm8p_try_launch takes (M >= 8192, 192 < N <= 256, K >= 4 * 64)
CHILD = r"""
import ctypes as C, hashlib, json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from roma_amd import _lib
lib = _lib.load("bf16")
M, N, K = 8192, 256, 256
g = np.random.Generator(np.random.PCG64(7))
A = torch.from_numpy(g.standard_normal(size=(M, K), dtype=np.float32)).cuda().bfloat16()
W = torch.from_numpy(g.standard_normal(size=(N, K), dtype=np.float32)).cuda().bfloat16()
P = lambda t: C.c_void_p(t.data_ptr())
def run():
    out = torch.empty((M, N), device="cuda", dtype=torch.bfloat16)
    assert lib.roma_profile_enable(1) == 0
    rc = lib.roma_op_gemm(P(A), K, P(W), K, P(out), N, M, N, K, 1, 0, 0, 0, None, None, None, 0, 0, 1.0, 1, 1, None)
    assert rc == 0, _lib.last_error(lib)
    torch.cuda.synchronize()
    n = lib.roma_profile_report(None, 0)
    buf = C.create_string_buffer(int(n))
    assert lib.roma_profile_report(buf, n) > 0
    assert lib.roma_profile_enable(0) == 0
    return {"kernels": sorted(json.loads(buf.value.decode())), "sha": hashlib.sha256(out.view(torch.int16).cpu().numpy().tobytes()).hexdigest()}
runs = [run()]
if len(sys.argv) > 2:  # then with the override
    assert lib.roma_tuning(b"gemm8p", int(sys.argv[2])) == 0
    runs.append(run())
print(json.dumps(runs))
"""


def child(env_extra, *args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ROMA_") or k == "ROMA_LIB_DIR"}
    env.update(env_extra)
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, *args], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode >= 0, "the child died on signal %d - nothing more is started\n%s" % (-run.returncode, run.stderr)
    assert run.returncode == 0, run.stderr
    return json.loads(run.stdout.strip().splitlines()[-1])


def test_environment_and_override_select_the_gemm_kernel():
    def on8p(r):
        return any(k.startswith("gemm8p_kernel<") for k in r["kernels"])

    (clean,) = child({})
    assert on8p(clean), clean
    env_off, overridden = child({"ROMA_GEMM8P": "0"}, "1")
    assert env_off["kernels"] and not on8p(env_off), env_off
    assert on8p(overridden), overridden
    assert clean["sha"] == env_off["sha"] == overridden["sha"]
