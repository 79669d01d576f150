"""What `training.normalize_observations` + `training.normalize_rewards` cost per update on TWO ranks that share one MI355X (peer transport, shared-GPU form).

    python tools/norm_ranks_rate.py [--out profiles/norm_ranks_rate.txt]

The supervisor starts two rank processes of this file (gloo rendezvous: RCCL refuses two ranks on one device, hipIpc does not).  Each process holds two
engines on the flagship configuration (`stompy_pro`, 4096 environments = 2 x 2048, float network) - one pair of ranks with both options off, one pair with
both on - and replays their captured updates.  After a warm-up the two pairs alternate: REPS rounds of UPDATES updates each, every round behind a barrier
and timed on rank 0 with device events around work that ends in a synchronise.  What to compare: across ranks the options add, to the T + 3 launches of
one rank, two rank-sum launches and one gather launch per update (one link round trip inside it).  The two pairs train on different inputs from the first
update on, so their environment steps are not the same work: the spread between rounds of ONE pair is printed beside the difference."""
import argparse
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

N, UPDATES, REPS, WARMUP, WORLD = 4096, 20, 7, 5, 2
NORM = ["training.normalize_observations=true", "training.normalize_rewards=true"]


def rank_main(rank: int, port: int, out_path: str) -> None:
    import numpy as np
    import torch
    import torch.distributed as dist

    from minppo_amd.config import load_config_from_cli
    from minppo_amd.train import Trainer

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    trainers = {}
    for name, extra in (("off", []), ("on", NORM)):
        tr = Trainer(load_config_from_cli(["stompy_pro", f"training.num_envs={N}", *extra]), device="cuda:0", rank=rank, world_size=WORLD, use_graph=True,
                     norm_after_connect=True)
        assert tr.init_comm("peer") == "peer" and tr.peer_form() == "shared", (tr.comm_mode(), tr.peer_form(), tr.comm_note)
        tr.reset()
        for _ in range(WARMUP):
            tr.update()
        tr._sync()
        assert tr.graph_active()
        trainers[name] = tr

    def timed(tr):
        dist.barrier()
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
    for tr in trainers.values():
        tr.check_peers()
        tr.check_replicas()
        tr.check_status()
    if rank == 0:
        on = trainers["on"]
        T = on.T
        with open(out_path, "w") as out:
            def say(*a):
                line = " ".join(str(x) for x in a)
                print(line, flush=True)
                out.write(line + "\n")

            say(f"# stompy_pro, {WORLD} ranks sharing one MI355X (peer transport, form {on.peer_form()}), {N} environments = {WORLD} x {on.N}, {T} steps, {on.E} epochs x {on.M} "
                f"minibatches, float network; captured graph replayed; {REPS} alternating rounds of {UPDATES} updates after {WARMUP} warm-up updates each; rank 0's device "
                "events around work that ends in a synchronise, every round behind a barrier")
            for name in ("off", "on"):
                m = np.median(us[name])
                say(f"normalize_observations + normalize_rewards {name:3s}  us/update: " + " ".join(f"{x:.1f}" for x in us[name])
                    + f"   median {m:.1f}   min .. max {min(us[name]):.1f} .. {max(us[name]):.1f}   -> {N * T / m:.3f} M env-steps/s")
            d = np.median(us["on"]) - np.median(us["off"])
            say(f"difference (medians)  us/update: {d:+.1f}   ({T} observation apply launches, 1 reward apply launch, 2 rank-sum launches, 1 gather launch, 2 merge launches "
                f"= {T + 6} launches more: {d / (T + 6):+.2f} us per added launch)")
            o, r = on.obs_norm(), on.reward_norm()
            say(f"statistics (replicas, checked): observation count {o['count']:.0f} (= {on.updates_done} updates x {T} x {on.N} x {WORLD}), return count {r['count']:.0f}, "
                f"scale {r['scale']:.4f}")
    dist.barrier()
    for tr in trainers.values():
        tr.close()
    dist.barrier()
    dist.destroy_process_group()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "norm_ranks_rate.txt"))
    ap.add_argument("--rank", type=int, default=-1)
    ap.add_argument("--port", type=int, default=0)
    args = ap.parse_args()
    if args.rank >= 0:
        rank_main(args.rank, args.port, args.out)
        return
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    procs = [subprocess.Popen([sys.executable, __file__, "--rank", str(r), "--port", str(port), "--out", args.out], env=env) for r in range(WORLD)]
    try:
        codes = [p.wait(timeout=540) for p in procs]
    finally:
        for p in procs:  # exactly the processes started above
            if p.poll() is None:
                p.kill()
                p.wait()
    sys.exit(max(abs(c) for c in codes))


if __name__ == "__main__":
    main()
