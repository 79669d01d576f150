"""What random pushes (`environment.push_force` > 0) cost per update and per environment step on one MI355X.

    python tools/push_rate.py [--out profiles/push_rate.txt]

Two engines in one process on the flagship configuration (`stompy_pro`: synth_stompy_pro, 4096 environments, float network), one with pushes off, one
with them on (a 0.1 s shove of up to 40 N on the torso every 2 s: the config's default interval and duration); both replay their captured update.  After
a warm-up the two alternate: REPS rounds of UPDATES updates each, every round timed with device events around work that ends in a synchronise.  Pushes add
no launch: what differs is the environment kernel's launch itself, which draws the wrench (two Philox blocks per lane) and projects it onto the dofs.  The
two engines' environments are in different states from the first push on, and the environment step's time depends on the states (contacts), so the spread
between rounds of ONE engine is printed beside the difference between the two.

Then the environment step on its own, in the manner of tools/env_time.py (walking states, 30 launches after 10, HIP events): mppo_env_step against
mppo_env_step_xfrc with a drawn wrench array, alternating, on the same states."""
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
PUSH = ["environment.push_force=40"]
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(ROOT / "profiles" / "push_rate.txt"))
out = open(ap.parse_args().out, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


trainers = {}
for name, extra in (("off", []), ("on", PUSH)):
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


us = {"off": [], "on": []}
for _ in range(REPS):  # alternating
    for name, tr in trainers.items():
        us[name].append(timed(tr))
on = trainers["on"]
T, env = on.T, on.config.environment
say(f"# stompy_pro, {N} environments x {T} steps, {on.E} epochs x {on.M} minibatches, float network; captured graph replayed; "
    f"{REPS} alternating rounds of {UPDATES} updates after {WARMUP} warm-up updates each; device events around work that ends in a synchronise")
say(f"# pushes: up to {env.push_force:g} N on body {on.push.body} for {env.push_duration} of every {env.push_interval} env steps (in any step {100.0 * env.push_duration / env.push_interval:.0f} % of the environments), drawn inside the step's launch")
for name in ("off", "on"):
    m = np.median(us[name])
    say(f"pushes {name:3s}  us/update: " + " ".join(f"{x:.1f}" for x in us[name]) + f"   median {m:.1f}   min .. max {min(us[name]):.1f} .. {max(us[name]):.1f}"
        f"   -> {N * T / m:.3f} M env-steps/s")
d = np.median(us["on"]) - np.median(us["off"])
say(f"difference (medians)  us/update: {d:+.1f}   = {d / T:+.2f} us per environment step launch ({100.0 * d / np.median(us['off']):+.2f} %)")
stats = {k: tr.rollout_stats() for k, tr in trainers.items()}
say("last rollout: " + "; ".join(f"pushes {k}: mean reward {v['mean_reward']:.4f}, {v['episodes']:.0f} episodes ended" for k, v in stats.items()))
lib, model, dims = on.lib, on._model, on.dims
for tr in trainers.values():
    tr.check_status()

# the environment step alone, on one set of walking states
s = torch.cuda.current_stream().cuda_stream
A = max(dims.nu, 1)
state0 = torch.zeros(N, dims.rec_dim, device="cuda")
reset, obs = torch.zeros(dims.rec_dim, device="cuda"), torch.zeros(N, dims.obs_pad, device="cuda")
rew, done = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
lib.env_reset(model, N, state0.data_ptr(), reset.data_ptr(), obs.data_ptr(), dims.obs_pad, 0, 0, None, s)
g = torch.Generator(device="cuda")
g.manual_seed(0)
acts = [torch.randn(N, A, device="cuda", generator=g) for _ in range(10)]
rc = on.ecfg.reward
xfrc = torch.zeros(N, 6, device="cuda")
always = nat.PushCfg(body=on.push.body, interval=1, duration=1, rank=0, force=float(env.push_force), seed=1)  # (every environment pushed: the dearest case)
sparse = nat.PushCfg(body=on.push.body, interval=int(env.push_interval), duration=int(env.push_duration), rank=0, force=float(env.push_force), seed=1)


def step(state, k, pushed):
    if pushed:
        lib.env_step_xfrc(model, N, 1, C.byref(rc), state.data_ptr(), reset.data_ptr(), acts[k % 10].data_ptr(), A, obs.data_ptr(), dims.obs_pad, rew.data_ptr(), done.data_ptr(),
                          None, on.push.body, xfrc.data_ptr(), s)
    else:
        lib.env_step(model, N, 1, C.byref(rc), state.data_ptr(), reset.data_ptr(), acts[k % 10].data_ptr(), A, obs.data_ptr(), dims.obs_pad, rew.data_ptr(), done.data_ptr(), None, s)


for k in range(10):
    step(state0, k, False)
torch.cuda.synchronize()
res = {}
for rnd in range(5):  # alternating, every measurement from the same walking states
    for name, cfg in (("mppo_env_step", None), ("mppo_env_step_xfrc, 5 % of the rows non-zero", sparse), ("mppo_env_step_xfrc, every row non-zero", always)):
        if cfg is not None:
            lib.push_fill(C.byref(cfg), N, None, 0, 3, xfrc.data_ptr(), s)
        state = state0.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(30):
            step(state, k, cfg is not None)
        e1.record()
        torch.cuda.synchronize()
        res.setdefault(name, []).append(e0.elapsed_time(e1) / 30 * 1e3)
say(f"# environment step alone ({N} environments, walking states, 30 launches per figure, 5 alternating rounds), us per launch:")
for name, v in res.items():
    say(f"{name:48s} " + " ".join(f"{x:.1f}" for x in v) + f"   median {np.median(v):.1f}   min .. max {min(v):.1f} .. {max(v):.1f}")
for tr in trainers.values():
    tr.close()
out.close()
