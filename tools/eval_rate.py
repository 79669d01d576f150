"""What the policy evaluator costs per step, beside the training rollout of the same tree, on one MI355X.

    python tools/eval_rate.py [--out profiles/eval_rate.txt]

`mppo_evaluate` on synth_stompy_pro, 4096 environments x 1000 steps, record_envs 0, after a warm-up call, timed with device events around work
that ends in a synchronise; in the same process, alternating, the same number of steps through `mppo_engine_rollout` (100 calls of 10 steps,
eager launches like the evaluator's).  Deterministic first (the figure README quotes), then stochastic (one more launch per step: the noise
fill).  What to compare: the evaluator's extra launch per step (the accumulate kernel) at the launch floor of profiles/r03_a_launch_floor.txt."""
import argparse
import ctypes as C
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from minppo_amd import _native as nat
from minppo_amd import evaluate as ev
from minppo_amd.config import make_config
from minppo_amd.train import Trainer

N, K, T = 4096, 1000, 10
BASE = {"kscale_id": "5eb3cb7f23232298", "visualization": {"camera_name": "track"}}
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(ROOT / "profiles" / "eval_rate.txt"))
out = open(ap.parse_args().out, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


for stochastic in (False, True):
    cfg = make_config(BASE, [f"training.num_envs={N}", f"training.num_steps={T}", f"rl.num_env_steps={T}", f"evaluation.num_envs={N}", f"evaluation.num_steps={K}",
                             f"evaluation.deterministic={'false' if stochastic else 'true'}"])
    tr = Trainer(cfg, device="cuda:0", use_graph=False)
    tr.reset()
    lib, s = tr.lib, tr.stream
    ecfg = ev.eval_cfg(cfg, seed=tr.seed)
    need = int(lib.eval_ws_bytes(tr._model, C.byref(tr.net), C.byref(ecfg)))
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=tr.device)
    ws = ws[(-ws.data_ptr()) % 256:][:need]
    res = torch.zeros(12, dtype=torch.int64, device=tr.device)
    params = tr.region("params")
    torch.cuda.synchronize()

    def run_eval(k):
        e = nat.EvalCfg.from_buffer_copy(ecfg)
        e.K = k
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        lib.evaluate(tr._model, C.byref(tr.net), nat.ptr(params), C.byref(e), nat.ptr(ws), need, nat.ptr(res), None, s.cuda_stream)
        b.record(s)
        s.synchronize()
        return a.elapsed_time(b) * 1e3 / k  # us per step

    def run_rollout(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for _ in range(calls):
            lib.engine_rollout(tr._engine, s.cuda_stream)
        b.record(s)
        s.synchronize()
        return a.elapsed_time(b) * 1e3 / (calls * T)

    run_eval(50); run_rollout(5)  # warm-up: code objects, clocks
    ev_us, ro_us = [], []
    for _ in range(5):  # alternating
        ev_us.append(run_eval(K))
        ro_us.append(run_rollout(K // T))
    r = nat.EvalResultRaw.from_buffer_copy(res.cpu().numpy().tobytes())
    mode = "stochastic (one mppo_normal_fill launch per step)" if stochastic else "deterministic (zero noise buffer)"
    say(f"# {mode}: synth_stompy_pro, {N} environments x {K} steps, hidden 256, float network, record_envs 0; eager launches, device events around work that ends in a synchronise; 5 alternating repetitions after a warm-up call")
    say(f"mppo_evaluate        us/step: " + " ".join(f"{x:.2f}" for x in ev_us) + f"   median {np.median(ev_us):.2f}   -> {N / np.median(ev_us):.3f} M env-steps/s")
    say(f"mppo_engine_rollout  us/step: " + " ".join(f"{x:.2f}" for x in ro_us) + f"   median {np.median(ro_us):.2f}   ({K // T} calls of {T} steps, eager; each call also fills the noise, runs the bootstrap critic, GAE and the rollout statistics)")
    say(f"difference           us/step: {np.median(ev_us) - np.median(ro_us):+.2f}")
    say(f"result: episodes {r.episodes} survivors {r.survivors} steps {r.steps} reward_sum {r.reward_sum:.6f} ret_sum {r.ret_sum:.6f}")
    tr.close()
out.close()
