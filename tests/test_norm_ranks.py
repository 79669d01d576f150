"""`training.normalize_observations` / `training.normalize_rewards` on several ranks (DESIGN.md 3.7 "Across ranks"): every rank adds its own partial sums
in index order (`mppo_obs_norm_rank_sums`), the ranks' slots are gathered once per update - the peer exchange's `peer_gather_f64_kernel` or one float64
all-reduce in which every foreign term is +0.0 - and `mppo_obs_norm_update` adds them in rank order and merges k = T N G rows.

The oracle is the float64 NumPy restatement of tests/test_obs_norm.py (imported: index-order sums, Chan's merge operation by operation, the float32 table)
in front of which `ref_rank_sums` restates the new stage.  Everything here that compares ranks with their own partials is bit for bit: the sums have one
order, the merge is a dozen IEEE operations compiled without contraction.  Ranks against ONE process on the union of the shards differ by float64
summation order: |mean|, |M2| within 1e-12 sum|d| per column (64 to 256 terms at 1.1e-16 each), the table within one float32 ulp, the count exact.

Rank processes: tests/norm_ranks_worker.py (emulator: shared-memory transports; -m gpu: 2 and 4 processes sharing cuda:0, the gather inside each rank's
captured graph)."""
import functools
import os
import pickle
import socket
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

from backends import get_backend
from dist_worker import make_inputs
from minppo_amd import train as T
from minppo_amd.config import make_config
from minppo_amd.evaluate import evaluate
from test_obs_norm import _ulps, ref_partials, ref_update  # the restatement, by import

f32, f64 = np.float32, np.float64
HERE = Path(__file__).resolve().parent
BASE = {"kscale_id": "5eb3cb7f23232298", "visualization": {"camera_name": "track"}}
EPS = f32(1e-8)
NORM = ["training.normalize_observations=true", "training.normalize_rewards=true", "training.obs_norm_clip=0", "training.reward_norm_clip=0"]
OVR = ["training.num_envs=8", "training.num_steps=4", "rl.num_env_steps=4", "training.num_minibatches=2", "training.update_epochs=2", "model.hidden_size=32",
       "training.total_timesteps=3200"] + NORM
GPU_OVR = ["training.num_envs=256", "training.num_minibatches=4", "training.update_epochs=2", "training.total_timesteps=100000000"] + NORM
SENTINEL = 123.5


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def ref_rank_sums(partials):
    """partials [P, 2, O] -> this rank's slot [2, O]: index order from +0.0 (as the update kernel adds them), a -0.0 sum published as +0.0."""
    S = np.zeros(partials.shape[1:], f64)
    for p in partials:
        S = S + p
    return np.where(S == 0.0, 0.0, S)


def ref_gathered_update(rank_partials, rows, stats, mean32, O):
    """rank_partials: per rank [P, 2, O].  Rank sums -> slots in rank order -> the merge of `rows` rows -> (stats', table' [2, O])."""
    slots = np.stack([ref_rank_sums(p) for p in rank_partials])
    return ref_update(slots, rows, np.asarray(stats, f64), np.asarray(mean32, f32), EPS, O)


# ---- 1: the stage against its restatement ----------------------------------------------------------------------------------------------------------


def _run_rank_sums(be, partials, rank, world):
    """-> slots [world, 2, O]; the buffer has one slab more in front and behind, which must stay untouched."""
    P, _, O = partials.shape
    buf = be.full((world + 2, 2, O), SENTINEL, f64)
    pdev = be.arr(partials)
    be.lib.obs_norm_rank_sums(O, P, be.ptr(pdev), rank, world, be.ptr(buf) + 8 * 2 * O, be.stream)
    be.sync()
    out = be.host(buf)
    assert (out[0] == SENTINEL).all() and (out[world + 1] == SENTINEL).all(), "words outside the slots were written"
    return out[1:world + 1].copy()


def _hand_made(P, O, seed):
    rng = np.random.default_rng(seed)
    part = rng.standard_normal((P, 2, O)) * rng.choice([1e-3, 1.0, 1e6], O)[None, None, :]
    part[:, 1] = np.abs(part[:, 1])
    part[:, 0, 0] = -0.0  # a column whose terms are all -0.0 ...
    if O > 1 and P > 1:  # ... and one that cancels exactly
        part[:, 0, 1] = 0.0
        part[0, 0, 1], part[P - 1, 0, 1] = 2.5, -2.5
    return part.astype(f64)


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2), (2, 3), (7, 8)])
@pytest.mark.parametrize("O", [1, 5, 225])
@pytest.mark.parametrize("P", [1, 6])
def test_rank_sums_is_the_restatement_bit_for_bit(be, P, O, rank, world):
    part = _hand_made(P, O, 1000 * P + O + world)
    slots = _run_rank_sums(be, part, rank, world)
    want = ref_rank_sums(part)
    assert np.array_equal(_bits(slots[rank]), _bits(want))
    assert slots[rank].view(np.uint64)[0, 0] == 0, "a sum of -0.0 terms is published as +0.0"
    for q in range(world):
        if q != rank:
            assert (slots[q].view(np.uint64) == 0).all(), f"foreign slot {q} is not +0.0"
    # under a sum all-reduce the foreign zeros change nothing: the gathered buffer is the ranks' own bits
    if world > 1:
        others = [_hand_made(P, O, 77 + q) for q in range(world)]
        bufs = [_run_rank_sums(be, others[q], q, world) for q in range(world)]
        total = bufs[0]
        for b in bufs[1:]:
            total = total + b
        assert np.array_equal(_bits(total), _bits(np.stack([ref_rank_sums(o) for o in others])))


@pytest.mark.parametrize("O,table_ld", [(1, 1), (5, 8), (225, 228)])
@pytest.mark.parametrize("P", [1, 6])
def test_one_rank_composition_gives_the_bytes_of_the_update_on_the_partials(be, P, O, table_ld):
    """rank_sums(world = 1) then update(n_partials = 1) == update(n_partials = P) on the original partials: statistics and table alike."""
    rng = np.random.default_rng(P * 10 + O)
    mean32 = rng.standard_normal(O).astype(f32)
    x = (mean32[None, :] + rng.standard_normal((P * 128, O)) * rng.choice([0.1, 1.0, 30.0], O)[None, :]).astype(f32)
    part = ref_partials(x, mean32)
    assert part.shape == (P, 2, O)
    rows = P * 128
    stats0 = np.concatenate([[50.0], rng.standard_normal(O), 50.0 * rng.uniform(0.5, 2.0, O)])

    def update(partials):
        tab = np.full((2, table_ld), 55.5, f32)
        tab[0, :O], tab[1, :O] = mean32, 1.0
        sdev, tdev, pdev = be.arr(stats0), be.arr(tab), be.arr(partials)
        be.lib.obs_norm_update(O, len(partials), rows, be.ptr(pdev), be.ptr(sdev), float(EPS), be.ptr(tdev), table_ld, be.stream)
        be.sync()
        return be.host(sdev).copy(), be.host(tdev).copy()

    direct = update(part)
    composed = update(_run_rank_sums(be, part, 0, 1))
    assert np.array_equal(_bits(direct[0]), _bits(composed[0])) and np.array_equal(_bits(direct[1]), _bits(composed[1]))
    want_stats, want_table = ref_gathered_update([part], rows, stats0, mean32, O)
    assert np.array_equal(_bits(composed[0]), _bits(want_stats)) and np.array_equal(_bits(composed[1][:, :O]), _bits(want_table))


def test_rank_sums_refuses_bad_arguments(be):
    f = be.lib._fn["mppo_obs_norm_rank_sums"]
    part, slots = be.zeros((2, 2, 5), f64), be.zeros((2, 2, 5), f64)
    assert f(5, 2, be.ptr(part), 2, 2, be.ptr(slots), be.stream) == -1 and "rank 2 of 2" in be.lib.last_error()
    assert f(5, 2, be.ptr(part), -1, 2, be.ptr(slots), be.stream) == -1 and f(5, 2, be.ptr(part), 0, 0, be.ptr(slots), be.stream) == -1
    assert f(0, 2, be.ptr(part), 0, 2, be.ptr(slots), be.stream) == -1 and f(5, 0, be.ptr(part), 0, 2, be.ptr(slots), be.stream) == -1
    assert f(5, 2, None, 0, 2, be.ptr(slots), be.stream) == -1 and f(5, 2, be.ptr(part), 0, 2, None, be.stream) == -1
    assert f(5, 2, be.ptr(part) + 4, 0, 2, be.ptr(slots), be.stream) == -1 and "aligned" in be.lib.last_error()


def test_dyadic_shards_equal_the_union_bit_for_bit(be):
    """Rows and mean on the grid of multiples of 2^-6 within +-8: every partial sum is exact in float64 in any order, so three ranks' shards through
    apply -> rank_sums -> (gather) -> update equal ONE process's apply -> update over all rows, statistics and table bit for bit."""
    O, ld, world, Nl = 7, 8, 3, 150  # (two apply workgroups per rank, the second a part)
    rng = np.random.default_rng(5)
    x = (rng.integers(-512, 513, (world * Nl, O)) / 64.0).astype(f32)
    mean32 = (rng.integers(-512, 513, O) / 64.0).astype(f32)
    table = np.stack([mean32, np.full(O, 0.5, f32)])
    stats0 = np.concatenate([[64.0], rng.integers(-64, 65, O) / 8.0, rng.integers(1, 65, O) * 2.0])

    def partials_of(rows):
        host = np.zeros((len(rows), ld), f32)
        host[:, :O] = rows
        dev, tdev = be.arr(host), be.arr(table)
        G = be.lib.obs_norm_partials(len(rows))
        part = be.zeros((G, 2, O), f64)
        be.lib.obs_norm_apply(len(rows), O, be.ptr(dev), ld, be.ptr(tdev), O, 0.0, be.ptr(part), be.stream)
        be.sync()
        return be.host(part).copy()

    def update(partials):
        sdev, tdev, pdev = be.arr(stats0), be.arr(table), be.arr(partials)
        be.lib.obs_norm_update(O, len(partials), world * Nl, be.ptr(pdev), be.ptr(sdev), float(EPS), be.ptr(tdev), O, be.stream)
        be.sync()
        return be.host(sdev).copy(), be.host(tdev).copy()

    union = update(partials_of(x))
    gathered = np.zeros((world, 2, O), f64)
    for r in range(world):
        gathered = gathered + _run_rank_sums(be, partials_of(x[r * Nl:(r + 1) * Nl]), r, world)
    ranks = update(gathered)
    assert ranks[0][0] == 64.0 + world * Nl
    assert np.array_equal(_bits(union[0]), _bits(ranks[0])) and np.array_equal(_bits(union[1]), _bits(ranks[1]))


# ---- 2, 5: ranks against their own partials ---------------------------------------------------------------------------------------------------------


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(world, updates, ovr, env, timeout, outdir):
    port = _free_port()
    procs = [subprocess.Popen([sys.executable, str(HERE / "norm_ranks_worker.py"), str(r), str(world), str(port), str(updates), str(Path(outdir) / f"r{r}.npz"), *ovr],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(world)]
    try:
        outs = [p.communicate(timeout=timeout)[0] for p in procs]  # (every rank process has its own limit)
    finally:
        for p in procs:  # exactly the PIDs started above
            if p.poll() is None:
                p.kill()
                p.wait()
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)  # (a peer wait that timed out raised in the worker's check_peers: never retried)
    return [dict(np.load(Path(outdir) / f"r{r}.npz")) for r in range(world)]


def _emu_ovr(world):
    return [o if not o.startswith("training.num_envs=") else f"training.num_envs={ {3: 12, 8: 16}.get(world, 8)}" for o in OVR]


@functools.lru_cache(maxsize=None)
def _emu_ranks(world, transport):
    """Two updates of `world` emulator ranks; run once per (world, transport) and shared by the tests below (never modified)."""
    env = dict(os.environ, MPPO_TEST_BACKEND="emu", MPPO_TEST_GRAPH="0", MPPO_ALLREDUCE="peer" if transport == "peer_selftest_fails" else transport)
    for k in ("MPPO_TEST_SELFTEST_FAIL_RANK", "MPPO_TEST_TABLE_MISMATCH", "MPPO_TEST_CKPT"):
        env.pop(k, None)
    if transport == "peer_selftest_fails":
        env["MPPO_TEST_SELFTEST_FAIL_RANK"] = "1"
    return _spawn(world, 2, _emu_ovr(world), env, 900, tempfile.mkdtemp(prefix="norm_ranks_"))


def _dims(ovr, world):
    cfg = make_config(BASE, ovr)
    return cfg, cfg.training.num_envs // world, cfg.training.num_steps


def _assert_ranks_equal_their_own_partials(ranks, world, updates, Nl, Tn, O, OP):
    """Every update: rank sums -> slots in rank order -> Chan's merge from the previous statistics, recomputed from the ranks' dumped partials; statistics
    and tables equal it, and each other, bit for bit on every rank."""
    rows = Tn * Nl * world
    for u in range(1, updates + 1):
        prev_s, prev_t = ranks[0][f"u{u - 1}_obs_norm_stats"], ranks[0][f"u{u - 1}_obs_norm_table"].reshape(2, OP)
        want_s, want_t = ref_gathered_update([r[f"u{u}_obs_norm_partials"].reshape(-1, 2, O) for r in ranks], rows, prev_s, prev_t[0, :O], O)
        assert want_s[0] == u * rows
        prev_rs, prev_rt = ranks[0][f"u{u - 1}_reward_norm_stats"], ranks[0][f"u{u - 1}_reward_norm_table"]
        want_rs, want_rt = ref_gathered_update([r[f"u{u}_reward_norm_partials"].reshape(-1, 2, 1) for r in ranks], rows, prev_rs, prev_rt[:1], 1)
        for q, r in enumerate(ranks):
            table = r[f"u{u}_obs_norm_table"].reshape(2, OP)
            assert np.array_equal(_bits(r[f"u{u}_obs_norm_stats"]), _bits(want_s)), (u, q)
            assert np.array_equal(_bits(table[:, :O]), _bits(want_t)) and (table[0, O:] == 0).all() and (table[1, O:] == 1).all(), (u, q)
            assert np.array_equal(_bits(r[f"u{u}_reward_norm_stats"]), _bits(want_rs)), (u, q)
            assert np.array_equal(_bits(r[f"u{u}_reward_norm_table"]), _bits(want_rt.reshape(-1))), (u, q)
        assert not (want_t[1] == 1).all() and want_rt[1, 0] != 1, "the tables are in use"
    for r in ranks[1:]:
        assert np.array_equal(_bits(ranks[0]["params"]), _bits(r["params"])), "parameter replicas differ"
    assert all(r["obs_count"] == updates * rows and r["reward_count"] == updates * rows for r in ranks), "count is the global count"
    # the carry is per environment: the ranks hold different returns
    assert not np.array_equal(ranks[0][f"u{updates}_reward_norm_carry"], ranks[1][f"u{updates}_reward_norm_carry"])


@pytest.mark.parametrize("world,transport", [(2, "peer"), (2, "rccl"), (3, "peer"), (3, "rccl"), (8, "peer"), (2, "peer_selftest_fails")])
def test_ranks_equal_the_merge_of_their_own_partials(world, transport):
    """"peer_selftest_fails": rank 1's connect-time self-test reports failure - all ranks drop the exchange and continue on the communicator."""
    ranks = _emu_ranks(world, transport)
    cfg, Nl, Tn = _dims(_emu_ovr(world), world)
    assert all(str(r["comm"]) == ("peer" if transport == "peer" else "rccl") for r in ranks)
    _assert_ranks_equal_their_own_partials(ranks, world, 2, Nl, Tn, 225, 228)


@pytest.mark.parametrize("world", [2, 3])
def test_both_transports_give_the_same_bits(world):
    """The first update's rollout runs before any optimizer step, so both transports are given the same partials: the gather must hand the merge the same
    bits (statistics, tables, and the -0.0 / +0.0 convention with them).  From the second update on the two transports' gradient sums differ in rounding
    and the rollouts with them; there each transport is held to its own partials (above)."""
    a, b = _emu_ranks(world, "peer"), _emu_ranks(world, "rccl")
    others = [_emu_ranks(world, "peer_selftest_fails")] if world == 2 else []
    for other in [b] + others:
        for r, q in zip(a, other):
            keys = [k for k in r if k.startswith(("u0_", "u1_"))]
            assert len(keys) >= 12
            for k in keys:
                assert np.array_equal(_bits(r[k]), _bits(q[k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_rank_processes_sharing_one_gpu(tmp_path, world):
    """`world` rank PROCESSES share cuda:0 (the shared-GPU form of the exchange), the rank sums, the gather and the merge inside every rank's captured
    graph: three updates, every rank's statistics and tables equal the merge recomputed from all ranks' dumped partials, bit for bit."""
    env = dict(os.environ, MPPO_TEST_BACKEND="hip", MPPO_TEST_GRAPH="1", MPPO_ALLREDUCE="peer", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    for k in ("MPPO_PEER_MODE", "MPPO_TEST_SELFTEST_FAIL_RANK", "MPPO_TEST_TABLE_MISMATCH", "MPPO_TEST_CKPT"):
        env.pop(k, None)
    ranks = _spawn(world, 3, GPU_OVR, env, 600, tmp_path)
    assert all(bool(r["graph"]) for r in ranks), "a rank did not replay its hipGraph"
    assert all(str(r["comm"]) == "peer" for r in ranks)
    cfg, Nl, Tn = _dims(GPU_OVR, world)
    _assert_ranks_equal_their_own_partials(ranks, world, 3, Nl, Tn, 225, 228)


# ---- 3: ranks against one process on the union ------------------------------------------------------------------------------------------------------


def _returns(reward, done, gamma):
    """The discounted returns the reward scaling counts ([T, N] float32, carry 0): ret = ret * gamma + reward, restarted behind a done."""
    ret, out = np.zeros(reward.shape[1], f32), np.zeros(reward.shape, f32)
    for t in range(reward.shape[0]):
        ret = ret * f32(gamma) + reward[t]
        out[t] = ret
        ret = np.where(done[t] != 0, f32(0), ret)
    return out


@pytest.mark.parametrize("world,transport", [(2, "peer"), (3, "rccl")])
def test_ranks_against_one_process_on_the_union(world, transport):
    ranks = _emu_ranks(world, transport)
    ovr = _emu_ovr(world)
    be = get_backend("emu")
    cfg = make_config(BASE, ovr)
    tr = be.trainer(cfg, external_random=True, use_graph=False)
    tr.reset()
    N, Tn, A, E, M, O, OP = tr.N, tr.T, tr.A, tr.E, tr.M, tr.O, tr.OP
    first = None
    for u in range(2):
        noise, _, glob = make_inputs(N, Tn, A, E, M, world, seed=100 + u)
        tr.region("noise", (Tn, N, A))[:] = noise
        tr.region("perm", (E, Tn * N))[:] = glob
        tr.update()
        if u == 0:
            first = {k: np.array(tr.region(k)) for k in ("obs_norm_stats", "obs_norm_table", "reward_norm_stats", "reward_norm_table", "reward", "done")}
            first["obs"] = np.array(tr.region("obs", (Tn + 1, N, OP)))
    # before any optimizer step the shards' rollouts are the union's slices (identity tables, no clamp: the stored rows are the raw ones)
    obs = first["obs"][1:, :, :O].astype(f64)
    assert np.array_equal(np.concatenate([r["u1_obs"][1:] for r in ranks], 1), first["obs"][1:])
    mag = np.abs(obs).sum((0, 1))  # sum |d| per column, d = x - 0
    got, want = ranks[0]["u1_obs_norm_stats"], first["obs_norm_stats"]
    assert got[0] == want[0] == Tn * N
    print("obs mean diff / bound max", (np.abs(got[1:1 + O] - want[1:1 + O]) / (1e-12 * mag + 1e-300)).max(), "M2", (np.abs(got[1 + O:] - want[1 + O:]) / (1e-12 * mag + 1e-300)).max())
    assert (np.abs(got[1:1 + O] - want[1:1 + O]) <= 1e-12 * mag).all() and (np.abs(got[1 + O:] - want[1 + O:]) <= 1e-12 * mag).all()
    assert _ulps(ranks[0]["u1_obs_norm_table"].reshape(2, OP)[:, :O], first["obs_norm_table"].reshape(2, OP)[:, :O]) <= 1
    rets = _returns(first["reward"].reshape(Tn, N), first["done"].reshape(Tn, N), cfg.rl.gamma)
    rmag = np.abs(rets.astype(f64)).sum()
    got, want = ranks[0]["u1_reward_norm_stats"], first["reward_norm_stats"]
    assert got[0] == want[0] == Tn * N
    print("return mean diff / bound", abs(got[1] - want[1]) / (1e-12 * rmag), "M2", abs(got[2] - want[2]) / (1e-12 * rmag))
    assert abs(got[1] - want[1]) <= 1e-12 * rmag and abs(got[2] - want[2]) <= 1e-12 * rmag
    assert _ulps(ranks[0]["u1_reward_norm_table"][1:], first["reward_norm_table"][1:]) <= 1 and ranks[0]["u1_reward_norm_table"][0] == first["reward_norm_table"][0]
    # after the last update: the shards' rewards are the union's to rounding (the parameters drift by summation order after the first one)
    np.testing.assert_allclose(np.concatenate([r["reward"] for r in ranks], 1), np.array(tr.region("reward", (Tn, N))), atol=5e-3)
    tr.close()


# ---- 4: the surface ------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("option", ["training.normalize_observations=true", "training.normalize_rewards=true"])
def test_two_ranks_construct_and_the_options_wait_for_a_transport(be, option):
    """`Trainer(cfg, world_size=2, norm_after_connect=True)` constructs; the options are switched on in the engine by `init_comm`, once a transport is
    connected - before that the engine refuses them (the statistics would be one rank's) and `reset()` says what is missing."""
    tr = be.trainer(make_config(BASE, [o for o in OVR if o not in NORM] + [option]), world_size=2, rank=1, external_random=True, norm_after_connect=True)
    assert tr.world_size == 2 and (tr.obs_norm_on or tr.reward_norm_on)
    name = "mppo_engine_set_obs_norm" if tr.obs_norm_on else "mppo_engine_set_reward_norm"
    assert be.lib._fn[name](tr._engine, 1, 10.0, 1e-8) == -1 and "connect it first" in be.lib.last_error()
    with pytest.raises(RuntimeError, match="init_comm"):
        tr.reset()
    with pytest.raises(RuntimeError, match="learn_host_driven"):
        tr.learn_host_driven(lambda view: None)
    tr.close()
    plain = be.trainer(make_config(BASE, [o for o in OVR if o not in NORM]), world_size=2, rank=1, external_random=True)
    plain.reset()
    plain.rollout()  # (both options off: the rollout needs no communication on any rank count)
    plain._sync()
    plain.close()


def test_checkpoint_model_file_and_replica_check_at_two_ranks(tmp_path):
    """One run of two emulator ranks: a checkpoint after update 1 resumes bit-exactly in a second Trainer (statistics, tables, carry, parameters) and refuses
    another world size; rank 0's model file carries "obs_norm" with the global count and `evaluate` reads it; `check_replicas` raises on every rank when
    one rank's observation table is off by one ulp."""
    env = dict(os.environ, MPPO_TEST_BACKEND="emu", MPPO_TEST_GRAPH="0", MPPO_ALLREDUCE="peer", MPPO_TEST_TABLE_MISMATCH="1", MPPO_TEST_CKPT=str(tmp_path))
    env.pop("MPPO_TEST_SELFTEST_FAIL_RANK", None)
    ovr = [o for o in OVR if "obs_norm_clip" not in o]  # (the default clamp: the model file carries it)
    ranks = _spawn(2, 2, ovr, env, 900, tmp_path)
    for r in ranks:
        assert bool(r["mismatch_raised"]) and bool(r["world_refused"])
        for k in ("obs_norm_stats", "obs_norm_table", "reward_norm_stats", "reward_norm_table", "reward_norm_carry"):
            assert np.array_equal(_bits(r[f"resumed_{k}"]), _bits(r[f"u2_{k}"])), k
        assert np.array_equal(_bits(r["resumed_params"]), _bits(r["params"]))
    cfg = make_config(BASE, ovr)
    with open(tmp_path / "model.pkl", "rb") as f:
        tree = pickle.load(f)
    on = tree["obs_norm"]
    assert on["count"] == 2 * cfg.training.num_steps * cfg.training.num_envs and on["clip"] == 10.0  # updates x T x N of ALL ranks
    assert np.array_equal(on["mean"], ranks[1]["u2_obs_norm_table"].reshape(2, 228)[0, :225])  # (rank 1's table: the same replica)
    be = get_backend("emu")
    kw = dict(lib=be.lib, xp=be.xp, num_envs=8, num_steps=4, record_envs=2, deterministic=True)
    a = evaluate(cfg, str(tmp_path / "model.pkl"), **kw)
    b = evaluate(cfg, T.tree_to_flat(tree, 225, 10, 32), obs_norm=on, **kw)
    c = evaluate(cfg, T.tree_to_flat(tree, 225, 10, 32), **kw)
    assert np.array_equal(_bits(a.trajectory["action"]), _bits(b.trajectory["action"])) and not np.array_equal(a.trajectory["action"], c.trajectory["action"])


def test_one_rank_is_the_composition_of_todays_stages(be):
    """world_size = 1 with both options on: after each of two updates the engine's statistics and tables are mppo_obs_norm_update on the update's own partials
    (n_partials = T G and G, rows = T N) from the previous statistics - no rank-sum stage, no gather - and "norm_slots" is never written."""
    tr = be.trainer(make_config(BASE, [o if not o.startswith("training.num_envs=") else "training.num_envs=37" for o in OVR if "minibatches" not in o]
                                + ["training.num_minibatches=1"]), external_random=True)
    tr.reset()
    host = lambda name: np.array(tr._to_host(tr.region(name)))
    be.put(tr.region("norm_slots"), np.full(2 * 226, SENTINEL))
    N, Tn, O, OP = tr.N, tr.T, tr.O, tr.OP
    rng = np.random.default_rng(3)
    for u in range(2):
        prev = {k: host(k) for k in ("obs_norm_stats", "obs_norm_table", "reward_norm_stats", "reward_norm_table")}
        be.put(tr.region("noise", (Tn, N, tr.A)), rng.standard_normal((Tn, N, tr.A)).astype(f32))
        be.put(tr.region("perm", (tr.E, N * Tn)), np.stack([rng.permutation(N * Tn) for _ in range(tr.E)]).astype(np.int32))
        tr.update()
        tr._sync()
        for name, cols, ld in (("obs_norm", O, OP), ("reward_norm", 1, 1)):
            part = host(f"{name}_partials").reshape(-1, 2, cols)
            sdev, tdev, pdev = be.arr(prev[f"{name}_stats"]), be.arr(prev[f"{name}_table"]), be.arr(part)
            be.lib.obs_norm_update(cols, len(part), Tn * N, be.ptr(pdev), be.ptr(sdev), float(EPS), be.ptr(tdev), ld, be.stream)
            be.sync()
            assert np.array_equal(_bits(be.host(sdev)), _bits(host(f"{name}_stats"))) and np.array_equal(_bits(be.host(tdev)), _bits(host(f"{name}_table"))), (u, name)
            want_s, want_t = ref_update(part, Tn * N, prev[f"{name}_stats"], prev[f"{name}_table"].reshape(2, ld)[0, :cols], EPS, cols)
            assert np.array_equal(_bits(host(f"{name}_stats")), _bits(want_s)) and np.array_equal(_bits(host(f"{name}_table").reshape(2, ld)[:, :cols]), _bits(want_t)), (u, name)
    assert (host("norm_slots") == SENTINEL).all()
    assert tr.obs_norm()["count"] == 2 * Tn * N == tr.reward_norm()["count"]
    tr.close()
