"""What `training.normalize_rewards` costs per update on one MI355X.

    python tools/reward_norm_rate.py [--out profiles/reward_norm_rate.txt]

Two engines in one process on the flagship configuration (`stompy_pro`: synth_stompy_pro, 4096 environments, float network), one with the option off,
one with it on; both replay their captured update (`_update_step`).  After a warm-up the two alternate: REPS rounds of UPDATES updates each, every
round timed with device events around work that ends in a synchronise.  What to compare: the option adds 2 launches per update (the apply stage in
front of GAE, the merge of the statistics behind it) at the 1.5 - 2.3 us launch floor of profiles/r03_a_launch_floor.txt.  The two engines train on
different advantages from the second update on (that is what the option is for), so their environment steps - whose time depends on the states - are
not the same work: the spread between rounds of ONE engine is printed beside the difference between the two."""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from minppo_amd.config import load_config_from_cli
from minppo_amd.train import Trainer

N, UPDATES, REPS, WARMUP = 4096, 20, 7, 5
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(ROOT / "profiles" / "reward_norm_rate.txt"))
out = open(ap.parse_args().out, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


trainers = {}
for name, extra in (("off", []), ("on", ["training.normalize_rewards=true"])):
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
T = trainers["on"].T
G = trainers["on"].lib.reward_norm_partials(N)
say(f"# stompy_pro, {N} environments x {T} steps, {trainers['on'].E} epochs x {trainers['on'].M} minibatches, float network; captured graph replayed; "
    f"{REPS} alternating rounds of {UPDATES} updates after {WARMUP} warm-up updates each; device events around work that ends in a synchronise")
for name in ("off", "on"):
    m = np.median(us[name])
    say(f"normalize_rewards {name:3s}  us/update: " + " ".join(f"{x:.1f}" for x in us[name]) + f"   median {m:.1f}   min .. max {min(us[name]):.1f} .. {max(us[name]):.1f}"
        f"   -> {N * T / m:.3f} M env-steps/s")
d = np.median(us["on"]) - np.median(us["off"])
say(f"difference (medians)  us/update: {d:+.1f}   = {d / 2:+.2f} us per added launch (1 apply launch of {G} workgroups over {T} x {N} rewards + 1 merge launch over {G} partials)")
on = trainers["on"].reward_norm()
say(f"statistics: count {on['count']:.0f} (= {trainers['on'].updates_done} updates x {T} x {N}), mean return {on['mean']:.4f}, std {np.sqrt(on['var']):.4f}, "
    f"scale {on['scale']:.6f}, clip {on['clip']:g}")
for tr in trainers.values():
    tr.check_status()
    tr.close()
out.close()
