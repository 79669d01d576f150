"""What sensor noise (`environment.obs_noise_*`) and actuation latency (`environment.action_delay_*`) cost per update on one MI355X.

    python tools/sensor_rate.py [--out profiles/sensor_rate.txt] [--parent-lib LIB] [--part a|b|ab]

The estimate, written down before the first run: either option adds one launch per rollout step, T = 10 per update at the bench shape, at the
1.5 - 2 us launch floor of profiles/r03_a_launch_floor.txt up to the 5.7 us profiles/domain_rand_rate.txt saw for a near-empty launch.  The latency's kernel
moves 3 x 164 KB: nothing beside the launch, 20 - 57 us per update.  The noise's kernel reads and writes the live blocks of 4096 rows of 225 columns - up to
3.7 MB each way, about half of that under the default group scales, rows the step kernel has just written - say 1 - 3 us on top of its launch: 30 - 90 us per
update.  Both: 50 - 147 us on the 6.2 ms update (0.8 - 2.4 %).

(a) The off path, with `--parent-lib LIB` (libminppo_hip.so of the parent commit): `bench.py --gpus 1` on that library (tools/bench_with_lib.py) and on this
tree's, alternating, three runs each, every run a process of its own.  The rule of DESIGN.md 3.9 - 3.11: this tree's median must lie inside the parent's own
min .. max spread widened by that spread's width.

(b) The on path.  Four engines in one process on the flagship configuration (`stompy_pro`: synth_stompy_pro, 4096 environments, float network): options off,
noise only, latency only, both.  All replay their captured update.  After a warm-up they alternate: REPS rounds of UPDATES updates each, every round timed with
device events around work that ends in a synchronise.  The engines' environments are in different states, and the environment step's time depends on the states
(contacts), so the spread between rounds of ONE engine is printed beside the differences.  Then the two stages alone, 30 launches per figure, on the engine's
own shapes, as captured chains of 30 launches."""
import argparse
import ctypes as C
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np

N, UPDATES, REPS, WARMUP = 4096, 20, 7, 5
NOISE = ["environment.obs_noise_level=1"]
DELAY = ["environment.action_delay_min=0", "environment.action_delay_max=4"]
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(ROOT / "profiles" / "sensor_rate.txt"))
ap.add_argument("--parent-lib", default=None, help="libminppo_hip.so built from the parent commit: bench.py on it and on this tree's, alternating")
ap.add_argument("--bench-runs", type=int, default=3)
ap.add_argument("--part", default="ab", choices=["a", "b", "ab"])
args = ap.parse_args()
out = open(args.out, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


if "a" in args.part:  # before this process opens the GPU: every bench.py run is a process of its own
    import json
    import subprocess

    if not args.parent_lib:
        raise SystemExit("part a needs --parent-lib")
    bench_args = ["--gpus", "1", "--steps", "30", "--warmup", "5"]
    runs = {"parent": [], "this tree": []}
    for _ in range(args.bench_runs):
        for name, cmd in (("parent", [str(ROOT / "tools" / "bench_with_lib.py"), str(Path(args.parent_lib).resolve())]), ("this tree", ["bench.py"])):
            r = subprocess.run([sys.executable, *cmd, *bench_args], cwd=str(ROOT), capture_output=True, text=True, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                raise SystemExit(f"bench.py failed ({name}):\n{r.stderr[-2000:]}")
            runs[name].append(float(json.loads(line[-1])["value"]) / 1e6)
    say(f"# (a) off path: bench.py --gpus 1 --steps 30 --warmup 5, parent commit's library and this tree's alternating, {args.bench_runs} runs each, M env-steps/s")
    for name, v in runs.items():
        say(f"{name:10s} " + " ".join(f"{x:.3f}" for x in v) + f"   median {np.median(v):.3f}   min .. max {min(v):.3f} .. {max(v):.3f}")
    lo, hi = min(runs["parent"]), max(runs["parent"])
    w, med = hi - lo, float(np.median(runs["this tree"]))
    say(f"parent's spread widened by its width: {lo - w:.3f} .. {hi + w:.3f}; this tree's median {med:.3f}: {'inside' if lo - w <= med <= hi + w else 'OUTSIDE'}")

if "b" not in args.part:
    out.close()
    raise SystemExit(0)

import torch

from minppo_amd import _native as nat
from minppo_amd.config import load_config_from_cli
from minppo_amd.train import Trainer

say("# (b) on path")
trainers = {}
for name, extra in (("off", []), ("noise", NOISE), ("latency", DELAY), ("noise + latency", NOISE + DELAY)):
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
on = trainers["noise + latency"]
T = on.T
say(f"# stompy_pro, {N} environments x {T} steps, {on.E} epochs x {on.M} minibatches, float network; captured graph replayed; "
    f"{REPS} alternating rounds of {UPDATES} updates after {WARMUP} warm-up updates each; device events around work that ends in a synchronise")
say("# noise: " + " ".join(r.split(".", 1)[1] for r in NOISE) + f" ({int((on.obs_noise > 0).sum())} of {on.O} columns live under the default group scales); latency: "
    + " ".join(r.split(".", 1)[1] for r in DELAY))
for name in trainers:
    m = np.median(us[name])
    say(f"{name:16s} us/update: " + " ".join(f"{x:.1f}" for x in us[name]) + f"   median {m:.1f}   min .. max {min(us[name]):.1f} .. {max(us[name]):.1f}"
        f"   -> {N * T / m:.3f} M env-steps/s")
base = np.median(us["off"])
for name, lo, hi in (("noise", 30, 90), ("latency", 20, 57), ("noise + latency", 50, 147)):
    d = np.median(us[name]) - base
    say(f"{name:16s} - off (medians)  us/update: {d:+.1f}   = {d / T:+.2f} us per rollout step ({100.0 * d / base:+.2f} %)   estimated {lo} - {hi}: "
        f"{'inside' if lo <= d <= hi else 'below' if d < lo else 'ABOVE'}")
stats = {k: tr.rollout_stats() for k, tr in trainers.items()}
say("last rollout: " + "; ".join(f"{k}: mean reward {v['mean_reward']:.4f}, {v['episodes']:.0f} episodes ended" for k, v in stats.items()))
for tr in trainers.values():
    tr.check_status()

# the two stages alone, on the engine's shapes (the rows one rollout step wrote; the engine's own tables)
lib = on.lib
s = torch.cuda.current_stream().cuda_stream
O, OP, A = on.O, on.OP, on.A
obs = torch.randn(N, OP, device="cuda")
sig = on.region("obs_noise_scale").clone()
dense = torch.full((OP,), 0.1, device="cuda")
dense[O:] = 0
nc = nat.ObsNoiseCfg(seed=1, rank=0, reserved=0)
dc = nat.ActionDelayCfg(min=0, max=4, rank=0, reserved=0, seed=1)
delays = torch.zeros(N, dtype=torch.int32, device="cuda")
lib.action_delay_fill(C.byref(dc), N, delays.data_ptr(), s)
ts, ep = torch.zeros(N, dtype=torch.int32, device="cuda"), torch.full((N,), 9, dtype=torch.int32, device="cuda")
act, hist, app = torch.randn(N, A, device="cuda"), torch.zeros(4, N, A, device="cuda"), torch.zeros(N, A, device="cuda")
stages = (("mppo_obs_noise_apply, default group scales", lambda k: lib.obs_noise_apply(C.byref(nc), N, O, obs.data_ptr(), OP, sig.data_ptr(), None, 0, k, s)),
          ("mppo_obs_noise_apply, every column live", lambda k: lib.obs_noise_apply(C.byref(nc), N, O, obs.data_ptr(), OP, dense.data_ptr(), None, 0, k, s)),
          ("mppo_action_delay_apply", lambda k: lib.action_delay_apply(C.byref(dc), N, A, delays.data_ptr(), ts.data_ptr(), ep.data_ptr(), act.data_ptr(), A, hist.data_ptr(),
                                                                       app.data_ptr(), A, s)))


def delay_stage(n):  # the same kernel on more environments: how much of its cost is the launch's shape (160 workgroups at 4096 environments)
    d_, t_, e_ = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"), torch.full((n,), 9, dtype=torch.int32, device="cuda")
    lib.action_delay_fill(C.byref(dc), n, d_.data_ptr(), s)
    a_, h_, o_ = torch.randn(n, A, device="cuda"), torch.zeros(4, n, A, device="cuda"), torch.zeros(n, A, device="cuda")
    keep.append((d_, t_, e_, a_, h_, o_))
    return lambda k: lib.action_delay_apply(C.byref(dc), n, A, d_.data_ptr(), t_.data_ptr(), e_.data_ptr(), a_.data_ptr(), A, h_.data_ptr(), o_.data_ptr(), A, s)


keep = []
stages += tuple((f"mppo_action_delay_apply, {n} environments", delay_stage(n)) for n in (1024, 16384, 65536))
# (eager launches from Python are bound by the host's call overhead: each stage's chain of 30 dependent launches is captured once and replayed, as the engine replays its update)
side = torch.cuda.Stream()
graphs = {}
for name, fn in stages:
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        cs = torch.cuda.current_stream().cuda_stream
        s = cs
        for k in range(30):
            fn(k)
    graphs[name] = g
s = torch.cuda.current_stream().cuda_stream
res = {}
for rnd in range(6):  # alternating; the first round warms up and is dropped
    for name, g in graphs.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(10):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        if rnd > 0:
            res.setdefault(name, []).append(e0.elapsed_time(e1) / 300 * 1e3)
say(f"# the stages alone ({N} environments; a captured chain of 30 dependent launches, 10 replays per figure, 5 alternating rounds), us per launch:")
for name, v in res.items():
    say(f"{name:48s} " + " ".join(f"{x:.2f}" for x in v) + f"   median {np.median(v):.2f}   min .. max {min(v):.2f} .. {max(v):.2f}")
for tr in trainers.values():
    tr.close()
out.close()
