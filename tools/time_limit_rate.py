"""What an episode time limit (`environment.episode_length` > 0) costs per update on one MI355X.

    python tools/time_limit_rate.py [--out profiles/time_limit_rate.txt]

Three engines in one process on the flagship configuration (`stompy_pro`: synth_stompy_pro, 4096 environments, float network): one without a limit, one
with `environment.episode_length=1000` (Brax's default; staggered first episodes), and one with a limit nobody reaches (1000000, no stagger) - its
environments are in the states of the first engine's, bit for bit, so its difference is the added launches alone, while the second engine's also holds what
restarted environments do to the environment step's state-dependent time.  All replay their captured update.  After a warm-up they alternate:
REPS rounds of UPDATES updates each, every round timed with device events around work that ends in a synchronise.  The limit adds one launch per rollout
step (mppo_env_time_limit: two loads per environment, and the reset record's copy for the few that are truncated), one byte per sample in GAE and in the
rollout statistics.  The spread between rounds of ONE engine is printed beside the difference between the two.

Then the truncation launch on its own: 4096 environments none of which / all of which are truncated, HIP events around 200 launches."""
import argparse
import ctypes as C
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from minppo_amd import _native as nat
from minppo_amd.config import load_config_from_cli
from minppo_amd.train import Trainer

N, UPDATES, REPS, WARMUP = 4096, 20, 7, 5
LIMIT = ["environment.episode_length=1000"]
NEVER = ["environment.episode_length=1000000", "environment.episode_length_stagger=false"]
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(ROOT / "profiles" / "time_limit_rate.txt"))
out = open(ap.parse_args().out, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


trainers = {}
for name, extra in (("off", []), ("on", LIMIT), ("never reached", NEVER)):
    tr = Trainer(load_config_from_cli(["stompy_pro", f"training.num_envs={N}", *extra]), device="cuda:0", use_graph=True)
    tr.reset()
    for _ in range(WARMUP):
        tr.update()
    tr._sync()
    assert tr.graph_active()
    trainers[name] = tr


def timed(tr):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(tr.stream)
    for _ in range(UPDATES):
        tr.update()
    b.record(tr.stream)
    tr.stream.synchronize()
    return a.elapsed_time(b) * 1e3 / UPDATES  # us per update


us = {k: [] for k in trainers}
truncated = 0.0
for _ in range(REPS):  # alternating
    for name, tr in trainers.items():
        us[name].append(timed(tr))
    truncated += trainers["on"].rollout_stats()["truncated"]
on = trainers["on"]
T, env = on.T, on.config.environment
say(f"# stompy_pro, {N} environments x {T} steps, {on.E} epochs x {on.M} minibatches, float network; captured graph replayed; "
    f"{REPS} alternating rounds of {UPDATES} updates after {WARMUP} warm-up updates each; device events around work that ends in a synchronise")
say(f"# time limit: environment.episode_length = {env.episode_length}, stagger {'on' if env.episode_length_stagger else 'off'}: one launch more per rollout step "
    f"({T} per update), GAE and the statistics read one byte more per sample; {truncated:.0f} truncations in the last rollouts of the {REPS} rounds")
for name in trainers:
    m = np.median(us[name])
    say(f"limit {name:13s}  us/update: " + " ".join(f"{x:.1f}" for x in us[name]) + f"   median {m:.1f}   min .. max {min(us[name]):.1f} .. {max(us[name]):.1f}"
        f"   -> {N * T / m:.3f} M env-steps/s")
for name in ("never reached", "on"):
    d = np.median(us[name]) - np.median(us["off"])
    say(f"limit {name} - off (medians)  us/update: {d:+.1f}   = {d / T:+.2f} us per rollout step ({100.0 * d / np.median(us['off']):+.2f} %)")
same = all(np.array_equal(trainers["off"]._to_host(trainers["off"].region(k)), trainers["never reached"]._to_host(trainers["never reached"].region(k))) for k in ("params", "state"))
say(f"limit never reached: parameters and environment states equal the engine's without a limit, bit for bit: {same}")
stats = {k: tr.rollout_stats() for k, tr in trainers.items()}
say("last rollout: " + "; ".join(f"limit {k}: mean reward {v['mean_reward']:.4f}, {v['episodes']:.0f} episodes ended" for k, v in stats.items()))
lib, model, dims = on.lib, on._model, on.dims
for tr in trainers.values():
    tr.check_status()

# the truncation launch alone
s = torch.cuda.current_stream().cuda_stream
state, rec, obs = torch.zeros(N, dims.rec_dim, device="cuda"), torch.zeros(dims.rec_dim, device="cuda"), torch.zeros(N, dims.obs_pad, device="cuda")
done, trunc = torch.zeros(N, dtype=torch.uint8, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
f32z = lambda: torch.zeros(N, device="cuda")
i32 = lambda v: torch.full((N,), v, dtype=torch.int32, device="cuda")
res = {}
for name, length in (("nobody truncated", 0), ("everybody truncated", 1000)):
    rows = []
    for rnd in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        lens = [i32(length) for _ in range(200)]  # (a truncation zeroes the lengths: a fresh array per launch)
        met = [f32z(), None, f32z(), i32(0), i32(5000), torch.zeros(N, dtype=torch.uint8, device="cuda")]
        cfg = nat.TimeLimitCfg(length=1000, stagger=1, rank=0, reserved=0, seed=1)
        torch.cuda.synchronize()
        e0.record()
        for k in range(200):
            met[1] = lens[k]
            ms = nat.EnvMetrics(*[x.data_ptr() for x in met])
            done.zero_()
            lib.env_time_limit(model, N, C.byref(cfg), state.data_ptr(), rec.data_ptr(), obs.data_ptr(), dims.obs_pad, done.data_ptr(), trunc.data_ptr(), C.byref(ms), s)
        e1.record()
        torch.cuda.synchronize()
        assert bool(trunc.all()) == (length > 0) and bool(trunc.any()) == (length > 0)
        rows.append(e0.elapsed_time(e1) / 200 * 1e3)
    res[name] = rows
say(f"# mppo_env_time_limit alone ({N} environments, 200 launches per figure, each behind a {N}-byte fill kernel, 5 rounds), us per pair of launches:")
for name, v in res.items():
    say(f"{name:24s} " + " ".join(f"{x:.1f}" for x in v) + f"   median {np.median(v):.1f}   min .. max {min(v):.1f} .. {max(v):.1f}")
for tr in trainers.values():
    tr.close()
out.close()
