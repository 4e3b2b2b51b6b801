"""What one match() enqueues, as JSON (GPU box): for every amp mode (f32, bf16, mixed) and stream count (1, 2) the trace
stage names and checksums of each sub-batch slot in order, the per-kernel launch counts of roma_profile_report and a SHA-256
of the returned warp and certainty.  Two builds schedule the same work when their dumps are equal: run it once per build
(ROMA_LIB_DIR selects the libraries) and compare.

    python tools/schedule_dump.py --out new.json
    ROMA_LIB_DIR=/path/to/other/build python tools/schedule_dump.py --out old.json
    python tools/schedule_dump.py --compare old.json new.json
    python tools/schedule_dump.py --golden tests/golden/trace_stage_names.json   # the names tests/test_gpu_trace.py pins
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--compare", nargs=2, default=None, metavar=("A", "B"))
ap.add_argument("--golden", default=None, help="write the slot-0 stage names of the tiny test shape (f32, bf16) instead")
args = ap.parse_args()

if args.compare:
    a, b = (json.load(open(f)) for f in args.compare)
    bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
    print(f"{len(a)} / {len(b)} configurations; differing: {bad if bad else 'none'}")
    sys.exit(1 if bad else 0)

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roma_amd import roma_model, synthetic  # noqa: E402

AMP = {"f32": (torch.float32, None), "bf16": (torch.bfloat16, None), "mixed": (torch.bfloat16, torch.float16)}
sd, dsd = synthetic.make_matcher_state_dict(0), synthetic.make_dinov2_state_dict(0)


def one(mode, max_batch, streams, profile):
    amp, dec = AMP[mode]
    inp = {k: v.cuda() for k, v in synthetic.make_inputs(max_batch, 112, 168, seed=7).items()}
    m = roma_model((112, 112), True, device="cuda:0", weights=sd, dinov2_weights=dsd, amp_dtype=amp, symmetric=True,
                   upsample_res=(168, 168), max_batch=max_batch, decoder_dtype=dec)
    lib = m._lib
    m.dual_stream = streams == 2
    m.trace = True
    if profile:
        m._ensure_handle()  # a mixed handle loads the sibling library, whose launches the profile then counts too
        lib.roma_profile_enable(1)
    warp, cert = m.match(inp["im_A"], inp["im_B"], im_A_high_res=inp["im_A_high_res"], im_B_high_res=inp["im_B_high_res"])
    torch.cuda.synchronize()
    rec = {"slots": []}
    for slot in range(streams):
        names, sums = m.debug_trace(slot)
        rec["slots"].append({"names": list(names), "sums": [int(s) for s in sums]})
    if profile:
        n = lib.roma_profile_report(None, 0)
        buf = C.create_string_buffer(int(n))
        lib.roma_profile_report(buf, n)
        lib.roma_profile_enable(0)
        rec["calls"] = {k: v["calls"] for k, v in sorted(json.loads(buf.value.decode()).items())}
    rec["sha256"] = hashlib.sha256(warp.cpu().numpy().tobytes() + cert.cpu().numpy().tobytes()).hexdigest()
    return rec


if args.golden:
    out = {mode: one(mode, 2, 2, False)["slots"][0]["names"] for mode in ("f32", "bf16")}
    json.dump(out, open(args.golden, "w"), indent=0)
    print({k: len(v) for k, v in out.items()})
else:
    out = {f"{mode}_streams{ns}": one(mode, 3, ns, True) for mode in AMP for ns in (1, 2)}
    json.dump(out, open(args.out, "w"), indent=0, sort_keys=True)
    print({k: (sum(len(s["names"]) for s in v["slots"]), sum(v["calls"].values()), v["sha256"][:12]) for k, v in out.items()})
