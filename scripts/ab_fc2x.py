"""Dev tool: the two-slab FC2 / QKV seam (GPTEngine fc2x) off / on alternating in ONE process: ms per step of the 256-step loop at batch 64, 48 layers; N runs per variant"""
import os, sys, time, statistics, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wmar_amd.utils import synth
from wmar_amd.models.engine import GPTEngine
N = int(sys.argv[1]) if len(sys.argv) > 1 else 10
cfg = synth.TAMING_GPT
sd = synth.synth_gpt_state_fast(cfg, 0, "cuda", logit_scale=30.0)
eng = {"off": GPTEngine(cfg, sd, max_batch=64, fc2x=False), "on": GPTEngine(cfg, sd, max_batch=64, fc2x=True)}
del sd
for k, e in eng.items():
    info = e.plan_info(64)
    print(k, "fc2=", info["fc2"], "| qkv=", info["qkv"], "| device_bytes=", e.device_bytes, flush=True)
q = torch.empty(256, 64, 16384, device="cuda").exponential_(1)
cond = (torch.arange(64) * 37 % 1000).cuda()
res = {k: [] for k in eng}
toks = {}
for it in range(N + 1):
    for k in ("off", "on"):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        toks[k] = eng[k].generate(cond, 256, q, 1.0, 250, 0.92, None, use_graph=True)
        torch.cuda.synchronize(); ms = (time.perf_counter() - t0) / 256 * 1e3
        if it > 0:
            res[k].append(ms)
    print("round", it, " ".join("%s=%.4f" % (k, v[-1]) for k, v in res.items() if v), flush=True)
print("token agreement on/off: %.4f" % float((toks["on"] == toks["off"]).float().mean()))
med = {k: statistics.median(v) for k, v in res.items()}
mad = {k: statistics.median([abs(x - med[k]) for x in v]) for k, v in res.items()}
for k in res:
    print("%-4s n=%d median %.4f  MAD %.4f  min %.4f  max %.4f ms/step" % (k, len(res[k]), med[k], mad[k], min(res[k]), max(res[k])))
gain = med["off"] - med["on"]
print("gain %.4f ms/step = %.2f %%; 3 x MAD(off) = %.4f; accepted: %s" % (gain, 100 * gain / med["off"], 3 * mad["off"], gain > 3 * mad["off"]))
for role in ("qkv", "fc2", "fc1", "attn", "proj"):
    print("profile_role %-5s off %.2f us  on %.2f us" % (role, eng["off"].profile_role(role, 64), eng["on"].profile_role(role, 64)))
