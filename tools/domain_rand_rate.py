"""What domain randomisation (`environment.friction_scale_* / actuator_scale_* / added_mass_*`) costs per update and per environment step on one MI355X.

    python tools/domain_rand_rate.py [--out profiles/domain_rand_rate.txt] [--parent DIR]

(a) The off path, with `--parent DIR` (a built checkout of the parent commit): `bench.py --gpus 1` in DIR and in this tree, alternating, three runs each, every
run a process of its own.  The rule of DESIGN.md 3.9 / 3.10: this tree's median must lie inside the parent's own min .. max spread widened by that spread's width.

(b) The on path.

Three engines in one process on the flagship configuration (`stompy_pro`: synth_stompy_pro, 4096 environments, float network): ranges off; ranges on; and
ranges off with `environment.reset_noise_scale=0.01`, which pays the same one masked re-initialisation launch per rollout step and so splits the on path's
cost into "the launch" and "the randomised step kernel against the (split) unrandomised one".  All replay their captured update.  After a warm-up they
alternate: REPS rounds of UPDATES updates each, every round timed with device events around work that ends in a synchronise.  The engines' environments are
in different states, and the environment step's time depends on the states (contacts), so the spread between rounds of ONE engine is printed beside the
differences.

Then the environment step on its own, in the manner of tools/env_time.py (walking states, 30 launches after 10, HIP events): mppo_env_step against
mppo_env_step_domain under the identity table and under a drawn one, alternating, on the same states - and the masked mppo_env_reset_domain over an
all-zero and over the step's own `done`."""
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
RANGES = ["environment.friction_scale_min=0.5", "environment.friction_scale_max=1.25", "environment.actuator_scale_min=0.8", "environment.actuator_scale_max=1.2",
          "environment.added_mass_min=-1", "environment.added_mass_max=3"]
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(ROOT / "profiles" / "domain_rand_rate.txt"))
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py there and here, alternating")
ap.add_argument("--bench-runs", type=int, default=3)
args = ap.parse_args()
out = open(args.out, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


if args.parent:  # before this process opens the GPU: every bench.py run is a process of its own
    import json
    import subprocess

    runs = {"parent": [], "this tree": []}
    for _ in range(args.bench_runs):
        for name, tree in (("parent", args.parent), ("this tree", str(ROOT))):
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "30", "--warmup", "5"], cwd=tree, capture_output=True, text=True, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                raise SystemExit(f"bench.py failed in {tree}:\n{r.stderr[-2000:]}")
            runs[name].append(float(json.loads(line[-1])["value"]) / 1e6)
    say(f"# (a) off path: bench.py --gpus 1 --steps 30 --warmup 5, parent commit's build and this tree alternating, {args.bench_runs} runs each, M env-steps/s")
    for name, v in runs.items():
        say(f"{name:10s} " + " ".join(f"{x:.3f}" for x in v) + f"   median {np.median(v):.3f}   min .. max {min(v):.3f} .. {max(v):.3f}")
    lo, hi = min(runs["parent"]), max(runs["parent"])
    w, med = hi - lo, float(np.median(runs["this tree"]))
    say(f"parent's spread widened by its width: {lo - w:.3f} .. {hi + w:.3f}; this tree's median {med:.3f}: {'inside' if lo - w <= med <= hi + w else 'OUTSIDE'}")
    say("# (b) on path")

trainers = {}
for name, extra in (("off", []), ("on", RANGES), ("off + reset noise", ["environment.reset_noise_scale=0.01"])):
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
for _ in range(REPS):  # alternating
    for name, tr in trainers.items():
        us[name].append(timed(tr))
on = trainers["on"]
T = on.T
say(f"# stompy_pro, {N} environments x {T} steps, {on.E} epochs x {on.M} minibatches, float network; captured graph replayed; "
    f"{REPS} alternating rounds of {UPDATES} updates after {WARMUP} warm-up updates each; device events around work that ends in a synchronise")
say("# ranges on: " + " ".join(r.split(".", 1)[1] for r in RANGES) + f", payload on body {on.domain.mass_body}")
for name in trainers:
    m = np.median(us[name])
    say(f"{name:18s} us/update: " + " ".join(f"{x:.1f}" for x in us[name]) + f"   median {m:.1f}   min .. max {min(us[name]):.1f} .. {max(us[name]):.1f}"
        f"   -> {N * T / m:.3f} M env-steps/s")
base = np.median(us["off"])
for name in ("on", "off + reset noise"):
    d = np.median(us[name]) - base
    say(f"{name:18s} - off (medians)  us/update: {d:+.1f}   = {d / T:+.2f} us per rollout step ({100.0 * d / base:+.2f} %)")
d = np.median(us["on"]) - np.median(us["off + reset noise"])
say(f"on - (off + reset noise)  us/update: {d:+.1f}   = {d / T:+.2f} us per rollout step: the randomised step kernel against the unrandomised (split) one, the table reads")
stats = {k: tr.rollout_stats() for k, tr in trainers.items()}
say("last rollout: " + "; ".join(f"{k}: mean reward {v['mean_reward']:.4f}, {v['episodes']:.0f} episodes ended" for k, v in stats.items()))
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
body = on.domain.mass_body
ident = torch.tensor([[1.0, 1.0, 0.0, 0.0]], device="cuda").repeat(N, 1).contiguous()
drawn = torch.zeros(N, 4, device="cuda")
dc = nat.DomainCfg.from_buffer_copy(on.domain)
dc.seed, dc.rank = 1, 0
lib.domain_fill(C.byref(dc), N, drawn.data_ptr(), s)


def step(state, k, table):
    if table is not None:
        lib.env_step_domain(model, N, 1, C.byref(rc), state.data_ptr(), reset.data_ptr(), acts[k % 10].data_ptr(), A, obs.data_ptr(), dims.obs_pad, rew.data_ptr(), done.data_ptr(),
                            None, 0, None, table.data_ptr(), body, s)
    else:
        lib.env_step(model, N, 1, C.byref(rc), state.data_ptr(), reset.data_ptr(), acts[k % 10].data_ptr(), A, obs.data_ptr(), dims.obs_pad, rew.data_ptr(), done.data_ptr(), None, s)


for k in range(10):
    step(state0, k, None)
torch.cuda.synchronize()
res = {}
for rnd in range(5):  # alternating, every measurement from the same walking states
    for name, table in (("mppo_env_step", None), ("mppo_env_step_domain, identity table", ident), ("mppo_env_step_domain, drawn table", drawn)):
        state = state0.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(30):
            step(state, k, table)
        e1.record()
        torch.cuda.synchronize()
        res.setdefault(name, []).append(e0.elapsed_time(e1) / 30 * 1e3)
    for name, fill in (("mppo_env_reset_domain over a mask of zeros", 0), ("mppo_env_reset_domain over a mask with 1 % set", 1)):
        mask = (torch.rand(N, device="cuda", generator=g) < 0.01 * fill).to(torch.uint8)
        state = state0.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(30):
            lib.env_reset_domain(model, N, state.data_ptr(), None, obs.data_ptr(), dims.obs_pad, None, None, None, mask.data_ptr(), drawn.data_ptr(), body, 0.0, 0, 0, 0,
                                 None, None, 0, s)
        e1.record()
        torch.cuda.synchronize()
        res.setdefault(name, []).append(e0.elapsed_time(e1) / 30 * 1e3)
say(f"# environment step alone ({N} environments, walking states, 30 launches per figure, 5 alternating rounds), us per launch:")
for name, v in res.items():
    say(f"{name:48s} " + " ".join(f"{x:.1f}" for x in v) + f"   median {np.median(v):.1f}   min .. max {min(v):.1f} .. {max(v):.1f}")
for tr in trainers.values():
    tr.close()
out.close()
