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


def run_child(cmd, env_extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ROMA_") or k == "ROMA_LIB_DIR"}
    env.update(env_extra)
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert run.returncode >= 0, "the child died on signal %d - nothing more is started\n%s" % (-run.returncode, run.stderr)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    return run.stdout


def child(env_extra, *args):
    return json.loads(run_child([sys.executable, "-c", CHILD, ROOT, *args], env_extra).strip().splitlines()[-1])


def test_environment_and_override_select_the_gemm_kernel():
    def on8p(r):
        return any(k.startswith("gemm8p_kernel<") for k in r["kernels"])

    (clean,) = child({})
    assert on8p(clean), clean
    env_off, overridden = child({"ROMA_GEMM8P": "0"}, "1")
    assert env_off["kernels"] and not on8p(env_off), env_off
    assert on8p(overridden), overridden
    assert clean["sha"] == env_off["sha"] == overridden["sha"]


def test_refiner_input_wave_per_pixel_kernel_with_the_vector_kernel_switched_off():
    """refiner_input_kernel<T> (one wave per pixel) is what refiner_input_launch falls back to when a buffer is not 16-byte
    aligned, and no aligned case reaches it: test_refiner_input_grid_sample_warp runs the vector kernel for C = 512 / 256 / 64.
    ROMA_RI_VEC=0 is the documented A/B switch that turns the vector kernel off, so the same test - same shapes, same bounds -
    in a child with that environment runs the wave-per-pixel kernel for f32 and 16-bit at those three widths."""
    out = run_child([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "gpu",
                     os.path.join("tests", "test_gpu_ops.py") + "::test_refiner_input_grid_sample_warp"], {"ROMA_RI_VEC": "0"})
    assert "8 passed" in out and "skipped" not in out and "failed" not in out, out[-3000:]
