"""Worker for tests/test_norm_ranks.py: one rank of an env-sharded run with `training.normalize_observations` and `training.normalize_rewards` on
(emulator kernels and shared-memory transports by default; MPPO_TEST_BACKEND=hip: every rank on cuda:0).  After every update the rank dumps the partial
sums its rollout made, and the statistics and tables the engine merged from all ranks' sums; the test recomputes the merge from the dumps.

    norm_ranks_worker.py <rank> <world> <port> <updates> <out.npz> overrides...

Switches (environment): MPPO_ALLREDUCE (peer | rccl), MPPO_TEST_GRAPH=1 (replay the captured update), MPPO_TEST_SELFTEST_FAIL_RANK=<r> (rank r's connect-time
self-test reports failure: all ranks continue on the communicator), MPPO_TEST_TABLE_MISMATCH=1 (the last rank's observation table is moved by one ulp:
check_replicas must raise on every rank), MPPO_TEST_CKPT=<dir> (checkpoint after the first update, resume in a second Trainer, compare)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BASE = {"kscale_id": "5eb3cb7f23232298", "visualization": {"camera_name": "track"}}
NORM_REGIONS = ("obs_norm_stats", "obs_norm_table", "reward_norm_stats", "reward_norm_table")


def snapshot(tr, be):
    """Statistics, tables, this update's partials and the carry, as they stand in the arena."""
    tr._sync()
    out = {k: np.array(be.host(tr.region(k))) for k in NORM_REGIONS + ("obs_norm_partials", "reward_norm_partials", "reward_norm_carry")}
    return out


def connect(tr, rank):
    want = os.environ.get("MPPO_ALLREDUCE", "peer")
    fail_rank = os.environ.get("MPPO_TEST_SELFTEST_FAIL_RANK")
    if fail_rank is not None:
        want = "rccl"
        if int(fail_rank) == rank:
            real = tr.lib.engine_peer_selftest

            def failing(engine, stream, ok_ref):
                real(engine, stream, ok_ref)  # (collective: the peers wait for this rank's contribution)
                ok_ref._obj.value = 0

            tr.lib.engine_peer_selftest = failing
    got = tr.init_comm()
    assert got == want == tr.comm_mode(), (got, want, tr.comm_mode())


def feed(tr, be, rank, world, N, u):
    from dist_worker import make_inputs

    noise, local, _ = make_inputs(N, tr.T, tr.A, tr.E, tr.M, world, seed=100 + u)
    be.put(tr.region("noise", (tr.T, tr.N, tr.A)), noise[:, rank * tr.N:(rank + 1) * tr.N])
    be.put(tr.region("perm", (tr.E, tr.T * tr.N)), local[rank])


def step(tr, use_graph):
    if use_graph:
        tr.update()
    else:
        tr.rollout()
        tr.learn()
    tr._sync()


def run_rank(rank, world, port, overrides, updates, out_path):
    import torch.distributed as dist

    from backends import get_backend
    from minppo_amd.config import make_config

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)  # rendezvous on the CPU: the ranks may share one GPU
    be = get_backend(os.environ.get("MPPO_TEST_BACKEND", "emu"))
    use_graph = os.environ.get("MPPO_TEST_GRAPH") == "1"
    cfg = make_config(BASE, overrides)
    tr = be.trainer(cfg, rank=rank, world_size=world, external_random=True, use_graph=use_graph, norm_after_connect=True)
    connect(tr, rank)  # (init_comm: the transport, then the options in the engine)
    tr.reset()
    N = cfg.training.num_envs
    dump = {}
    for k, v in snapshot(tr, be).items():
        if k in NORM_REGIONS:
            dump[f"u0_{k}"] = v  # what the reset wrote: nothing counted, the identity tables
    ckpt_dir = os.environ.get("MPPO_TEST_CKPT")
    for u in range(updates):
        feed(tr, be, rank, world, N, u)
        step(tr, use_graph)
        for k, v in snapshot(tr, be).items():
            dump[f"u{u + 1}_{k}"] = v
        if u == 0:
            dump["u1_obs"] = np.array(be.host(tr.region("obs", (tr.T + 1, tr.N, tr.OP))))  # (rows 1 .. T: normalised with the identity = raw; row 0: the next update's)
            dump["u1_reward"] = np.array(be.host(tr.region("reward", (tr.T, tr.N))))
            dump["u1_done"] = np.array(be.host(tr.region("done", (tr.T, tr.N))))
            if ckpt_dir:
                tr.check_peers()
                tr.check_replicas()
                tr.save_checkpoint(f"{ckpt_dir}/ck.npz.rank{rank}")
                tr.barrier()
    tr.check_peers()  # (collective) a wait that ran into its limit raises here: never a retry
    tr.check_replicas()  # (collective) parameters, statistics and tables: bit-identical replicas
    if os.environ.get("MPPO_TEST_TABLE_MISMATCH") == "1":
        if rank == world - 1:
            t = np.array(be.host(tr.region("obs_norm_table"))).copy()
            t[3] = np.nextafter(t[3], np.float32(1e9))
            be.put(tr.region("obs_norm_table"), t)
        try:
            tr.check_replicas()
            raised = False
        except RuntimeError as exc:
            raised = "replicas differ" in str(exc) and "observation table" in str(exc)
        assert raised, f"rank {rank}: check_replicas did not raise"
        dump["mismatch_raised"] = np.array(True)
    dump.update(params=tr.params_flat(), reward=np.array(be.host(tr.region("reward", (tr.T, tr.N)))), graph=np.array(tr.graph_active()),
                comm=np.array(tr.comm_mode()), obs_count=np.array(tr.obs_norm()["count"]), reward_count=np.array(tr.reward_norm()["count"]))
    if ckpt_dir and rank == 0:
        from minppo_amd.train import save_model

        save_model(tr.params, f"{ckpt_dir}/model.pkl")
    dist.barrier()  # nobody unmaps an exchange buffer a peer might still read
    tr.close()
    dist.barrier()
    if ckpt_dir:  # a second Trainer resumes from the file written after update 1 and repeats update 2 .. : the same bits
        tr2 = be.trainer(cfg, rank=rank, world_size=world, external_random=True, use_graph=use_graph, norm_after_connect=True)
        connect(tr2, rank)
        tr2.load_checkpoint(f"{ckpt_dir}/ck.npz.rank{rank}")
        assert tr2.updates_done == 1
        for u in range(1, updates):
            feed(tr2, be, rank, world, N, u)
            step(tr2, use_graph)
        tr2.check_peers()
        tr2.check_replicas()
        for k, v in snapshot(tr2, be).items():
            dump[f"resumed_{k}"] = v
        dump["resumed_params"] = tr2.params_flat()
        try:  # (another world size is refused by the file's metadata, as before)
            other = be.trainer(cfg, rank=0, world_size=1, external_random=True, use_graph=False, num_envs_local=tr2.N)
            try:
                other.load_checkpoint(f"{ckpt_dir}/ck.npz.rank{rank}")
                dump["world_refused"] = np.array(False)
            except ValueError as exc:
                dump["world_refused"] = np.array("world_size" in str(exc))
            other.close()
        finally:
            dist.barrier()
            tr2.close()
            dist.barrier()
    np.savez(out_path, **dump)
    dist.destroy_process_group()


if __name__ == "__main__":
    run_rank(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[6:], int(sys.argv[4]), sys.argv[5])
