"""Reset noise: environments start, and restart after `done`, from qpos0 + U(-s, s) / qvel = U(-s, s) (reference env.py:87,115-121 with
`reset_noise_scale` > 0; train.py:135,142,163-165 for the keys) - `mppo_env_reinit`, the reset kernel's masked, noisy form, and the engine,
trainer and `HumanoidEnv` on top of it.

The noise words are held to the host restatements bit for bit (minppo_amd/jaxrng.py: `reset_noise` for the reference's threefry tree,
`reset_noise_philox` for the engine's own stream); the rest of the record to the kernel's own forward probe at the same state, bit for bit, and
to the float64 oracle at the tolerances the existing forward-parity tests use.  Sizes: N = 37 environments (not a multiple of the four
environments of a wave: surplus groups, a partial last workgroup), three robots: a library instantiation with its factor in registers, a
robot on the run-time-sized kernel, and the ball-joint humanoid (quaternion words in a free and a ball joint)."""

import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from minppo_amd import _native as nat
from minppo_amd import jaxrng
from minppo_amd.config import make_config
from minppo_amd.model import load_model
from oracle.env_oracle import metrics_step
from oracle.physics_oracle import Physics
from physics_harness import GOLDEN, METRIC_TYPES, SMOOTH_TOL, check_against_oracle, probe

f32 = np.float32
S = 0.01
N37 = 37
SEED, RANK, EVENT = 0x1234567890, 3, 11
KEY = np.array([0x9E3779B9, 12345], np.uint32)
MODELS = {"pro": "synth_stompy_pro",                                      # a library instantiation, Cholesky factor in registers
          "runtime": str(GOLDEN / "hand_leg.xml"),                        # no instantiation: the run-time-sized kernel
          "ball": str(GOLDEN / "ball_joints" / "ball_humanoid.xml")}      # quaternion words of a free and of a ball joint
BASE = {"kscale_id": "5eb3cb7f23232298", "visualization": {"camera_name": "track"}}
_CM = {}


def _cm(which):
    if which not in _CM:
        _CM[which] = load_model(MODELS[which])
    return _CM[which]


def _noise(impl, N, cm, key=KEY, event=EVENT, seed=SEED, rank=RANK, scale=S):
    """The host restatement: (dq [N, nq], dv [N, nv]) of stream `impl` (0 philox, 1 threefry)."""
    if impl == 1:
        return jaxrng.reset_noise(key, N, cm.nq, cm.nv, scale)
    return jaxrng.reset_noise_philox(seed, rank, event, N, cm.nq, cm.nv, scale)


def _reinit(be, h, dims, N, impl, mask=None, scale=S, state=None, obs=None, key=KEY, event=EVENT, seed=SEED, rank=RANK):
    """mppo_env_reinit on fresh (or given) state / observation arrays -> host copies (state, obs)."""
    state = be.zeros((N, dims.rec_dim)) if state is None else state
    obs = be.zeros((N, dims.obs_pad)) if obs is None else obs
    dkey = be.arr(np.asarray(key, np.uint32))
    ctr = be.arr(np.array([event - 4], np.int32))  # (the event is the device word plus the offset)
    dmask = None if mask is None else be.arr(np.asarray(mask, np.uint8))
    be.lib.env_reinit(h, N, be.ptr(state), be.ptr(obs), dims.obs_pad, be.ptr(dmask), scale, impl, seed, rank, be.ptr(dkey), be.ptr(ctr), 4, be.stream)
    be.sync()
    return be.host(state).copy(), be.host(obs).copy()


def _plain_reset(be, h, dims, N):
    state, rec, obs = be.zeros((N, dims.rec_dim)), be.zeros((dims.rec_dim,)), be.zeros((N, dims.obs_pad))
    be.lib.env_reset(h, N, be.ptr(state), be.ptr(rec), be.ptr(obs), dims.obs_pad, 0, 0, None, be.stream)
    be.sync()
    return be.host(state).copy(), be.host(rec).copy(), be.host(obs).copy()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


_RECORDS = {}


def _records(be, which, impl):
    """The noisy reset of N37 environments, computed once per (backend, robot, stream) and shared by the tests below (left unchanged)."""
    k = (be.name, which, impl)
    if k not in _RECORDS:
        cm = _cm(which)
        h, dims, keep = be.model(cm)
        state, obs = _reinit(be, h, dims, N37, impl)
        be.lib.model_close(h)
        _RECORDS[k] = (state, obs, dims)
    return _RECORDS[k]


# ---- 1: the noise words, bit for bit ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("which", list(MODELS))
def test_noise_words_equal_the_host_restatement(be, which, impl):
    cm = _cm(which)
    state, obs, dims = _records(be, which, impl)
    dq, dv = _noise(impl, N37, cm)
    assert np.abs(dq).max() <= S and np.abs(dv).max() <= S and np.abs(dq).max() > 0.5 * S
    q0 = np.asarray(cm.t["qpos0"], f32)
    assert np.array_equal(_bits(state[:, :cm.nq]), _bits((q0[None] + dq).astype(f32)))
    assert np.array_equal(_bits(state[:, cm.nq:cm.nq + cm.nv]), _bits(dv))
    rows = {state[n, :cm.nq + cm.nv].tobytes() for n in range(N37)}
    assert len(rows) == N37  # no two environments share a row
    # (quaternion words carry noise like every other word and stay unnormalised, as MJX leaves them)
    if which == "ball":
        from physics_harness import quaternion_joints

        for qa, _ in quaternion_joints(cm):
            assert (np.abs(np.linalg.norm(state[:, qa:qa + 4].astype(np.float64), axis=1) - 1.0) > 1e-6).any()


def test_host_restatements_are_the_reference_tree():
    """`jaxrng.reset_noise` is split(K, N)[n] -> split -> uniform(-s, s) in jaxrng's own primitives; another event, rank or seed of the Philox stream is
    another draw."""
    dq, dv = jaxrng.reset_noise(KEY, 5, 7, 6, S)
    kn = jaxrng.split(KEY, 5)[3]
    r1, r2 = jaxrng.split(kn)
    assert np.array_equal(dq[3], jaxrng.uniform(r1, 7, -S, S)) and np.array_equal(dv[3], jaxrng.uniform(r2, 6, -S, S))
    dq2, _ = jaxrng.reset_noise(None, 5, 7, 6, S, env_keys=jaxrng.split(KEY, 5))
    assert np.array_equal(dq, dq2)
    a = jaxrng.reset_noise_philox(1, 0, 0, 4, 9, 8, S)
    for other in ((1, 0, 1), (1, 1, 0), (2, 0, 0)):
        b = jaxrng.reset_noise_philox(*other, 4, 9, 8, S)
        assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
    assert np.abs(np.concatenate([a[0], a[1]], 1)).max() <= S
    # the host Philox behind it: the Random123 known answers of philox4x32-10 (kat_vectors: zeros, all ones, the digits of pi), and the restatement the
    # permutation tests use
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert tuple(int(np.asarray(x).reshape(-1)[0]) for x in jaxrng._philox4x32(*[[c] for c in ctr], *key)) == want
    from test_kernels_ppo import _philox4x32 as perm_philox

    c = [np.arange(5, dtype=np.uint64) * np.uint64(k) for k in (1, 77, 0x10001, 0xfffffff)]
    for x, y in zip(jaxrng._philox4x32(*c, 1337, 9), perm_philox(*c, 1337, 9)):
        assert np.array_equal(x, y)
    rng, act, srt, step = jaxrng.update_keys_step(KEY, 3, 2, 96)
    rng2, act2, srt2 = jaxrng.update_keys(KEY, 3, 2, 96)
    assert np.array_equal(rng, rng2) and np.array_equal(act, act2) and np.array_equal(srt, srt2) and step.shape == (3, 2)
    k = KEY
    for t in range(3):
        k = jaxrng.split(k)[0]
        k, st = jaxrng.split(k)
        assert np.array_equal(st, step[t])


def test_update_keys_kernel_writes_the_step_keys(be):
    T, E, rounds = 3, 2, jaxrng.permutation_rounds(96)
    rng = be.arr(KEY.copy())
    act, srt, stp = be.zeros((T, 2), np.uint32), be.zeros((E, rounds, 2), np.uint32), be.zeros((T, 2), np.uint32)
    be.lib.threefry_update_keys_step(be.ptr(rng), T, E, rounds, be.ptr(act), be.ptr(srt), be.ptr(stp), be.stream)
    want = jaxrng.update_keys_step(KEY, T, E, 96)
    for got, w in zip((rng, act, srt, stp), want):
        assert np.array_equal(be.host(got), w)


# ---- 2: the rest of the record is the kernel's own forward pass at that state -------------------------------------------------------------


@pytest.mark.parametrize("which", list(MODELS))
def test_record_is_the_forward_pass_at_the_noisy_state(be, which):
    cm = _cm(which)
    state, obs, dims = _records(be, which, 1)
    nq, nv, nb, O, OP = cm.nq, cm.nv, cm.nbody, dims.obs_dim, dims.obs_pad
    h, _, keep = be.model(cm)
    got = probe(be, h, cm, state[:, :nq], state[:, nq:nq + nv], np.zeros((N37, max(cm.nu, 1)), f32), np.zeros((N37, nv), f32))
    be.lib.model_close(h)
    o_ci = nq + nv
    o_cv = o_ci + 10 * (nb - 1)
    o_qa = o_cv + 6 * (nb - 1)
    assert o_qa + nv == O
    assert np.array_equal(_bits(state[:, o_ci:o_cv]), _bits(got["cinert"][:, 1:].reshape(N37, -1))), "cinert"
    assert np.array_equal(_bits(state[:, o_cv:o_qa]), _bits(got["cvel"][:, 1:].reshape(N37, -1))), "cvel"
    assert np.array_equal(_bits(state[:, o_qa:O]), _bits(got["qfrc_actuator"])), "qfrc_actuator"
    assert np.array_equal(_bits(state[:, OP:OP + nv]), _bits(got["qacc"])), "qacc_warmstart = qacc"
    assert np.array_equal(_bits(state[:, OP + nv]), _bits(got["subtree_com1"])), "subtree_com[1].x"
    assert (state[:, OP + nv + 1] == 0).all(), "time"
    assert (state[:, O:OP] == 0).all() and (state[:, OP + nv + 2:] == 0).all(), "padding"
    assert np.array_equal(_bits(obs), _bits(state[:, :OP])), "the observation is the record's first OP words"


# ---- 3: against the float64 oracle -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("which", list(MODELS))
def test_noisy_reset_follows_the_float64_oracle(be, which):
    """The forward pass at the noisy states at the tolerances the forward-parity tests hold these robots to (SMOOTH_TOL; rows 1e-5 / 5e-4 / 5e-4,
    half the environments well-conditioned, the solver's cost within 5e-2: tests/test_ball_joints.py, tests/test_equality.py), and the record's own
    words against Physics.pipeline_init at test_kernels_physics.py::test_forward_matches_oracle's tolerances for them."""
    cm = _cm(which)
    state, obs, dims = _records(be, which, 1)
    nq, nv, nb, O, OP = cm.nq, cm.nv, cm.nbody, dims.obs_dim, dims.obs_pad
    qpos, qvel = state[:, :nq].astype(np.float64), state[:, nq:nq + nv].astype(np.float64)
    states = (qpos, qvel, np.zeros((N37, cm.nu)), np.zeros((N37, nv)))
    ref, got, good = check_against_oracle(be, cm, states, which, SMOOTH_TOL, dict(efc_J=1e-5, efc_D=5e-4, efc_aref=5e-4), min_good=N37 // 2, strict_cost=True)
    d = Physics(cm.t).pipeline_init(qpos, qvel)
    o_ci = nq + nv
    o_cv = o_ci + 10 * (nb - 1)
    o_qa = o_cv + 6 * (nb - 1)
    for k, sl, r, tol in (("cinert", slice(o_ci, o_cv), d.cinert[:, 1:], 1e-5), ("cvel", slice(o_cv, o_qa), d.cvel[:, 1:], 1e-4),
                          ("qfrc_actuator", slice(o_qa, O), d.qfrc_actuator, 1e-5)):
        r = np.asarray(r).reshape(N37, -1)
        err = np.abs(state[:, sl] - r).max() / (np.abs(r).max() + 1e-6)
        assert err <= tol, (which, k, err)
    assert np.allclose(state[:, OP + nv], d.subtree_com[:, 1, 0], atol=1e-5)
    assert np.array_equal(np.asarray(d.qacc_warmstart), np.asarray(d.qacc))  # pipeline_init: the warm start is the forward pass's qacc
    rel = np.abs(state[:, OP:OP + nv] - d.qacc).max(1) / (np.abs(d.qacc).max(1) + 1e-9)
    assert np.median(rel[good]) <= 5e-3 and rel[good].max() <= 0.3, (which, np.median(rel[good]), rel[good].max())


# ---- 4: scale 0 is the old reset ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("which", list(MODELS))
def test_scale_zero_writes_the_reset_record(be, which):
    cm = _cm(which)
    h, dims, keep = be.model(cm)
    st0, rec, obs0 = _plain_reset(be, h, dims, N37)
    for impl in (0, 1):
        state, obs = _reinit(be, h, dims, N37, impl, scale=0.0)
        assert np.array_equal(_bits(state), _bits(np.tile(rec, (N37, 1)))) and np.array_equal(_bits(state), _bits(st0)) and np.array_equal(_bits(obs), _bits(obs0))
    be.lib.model_close(h)


# ---- 5: the mask --------------------------------------------------------------------------------------------------------------------------------

MASKS = {"none": [], "one_mid_wave": [5], "whole_wave": [8, 9, 10, 11], "last": [N37 - 1]}


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("pattern", list(MASKS))
@pytest.mark.parametrize("which", list(MODELS))
def test_mask_selects_the_environments(be, which, pattern, impl):
    cm = _cm(which)
    full_state, full_obs, dims = _records(be, which, impl)
    h, _, keep = be.model(cm)
    mask = np.zeros(N37, np.uint8)
    mask[MASKS[pattern]] = 1
    fill_s, fill_o = np.full((N37, dims.rec_dim), -7.25, f32), np.full((N37, dims.obs_pad), 3.5, f32)
    state, obs = _reinit(be, h, dims, N37, impl, mask=mask, state=be.arr(fill_s), obs=be.arr(fill_o))
    be.lib.model_close(h)
    on = mask != 0
    assert np.array_equal(_bits(state[~on]), _bits(fill_s[~on])) and np.array_equal(_bits(obs[~on]), _bits(fill_o[~on])), "rows masked out keep their bytes"
    assert np.array_equal(_bits(state[on]), _bits(full_state[on])) and np.array_equal(_bits(obs[on]), _bits(full_obs[on])), "rows masked in are the unmasked launch's"


def test_reinit_leaves_reward_done_and_metrics_alone(be):
    """mppo_env_reinit takes neither reward, done nor metrics: what a step wrote there stays.  Held here on the arrays a step produced."""
    cm = _cm("pro")
    out = _step_and_reinit(be, cm, N=8, steps=1, impl=1)
    assert out["metrics_after"] == out["metrics_step"] and out["reward_after"] == out["reward_step"] and out["done_after"] == out["done_step"]


# ---- 6: step + reinit = the reference's step -------------------------------------------------------------------------------------------------


def _step_and_reinit(be, cm, N, steps, impl):
    """A reset and `steps` x (mppo_env_step, mppo_env_reinit(mask = done)) under a reward window that ends every episode at every step
    (height_min_z above the start height) -> per step: state, obs, done, and the bytes of reward / done / metrics after the step and after the reinit."""
    h, dims, keep = be.model(cm)
    OP, R, nu = dims.obs_pad, dims.rec_dim, max(cm.nu, 1)
    state, rec, obs = be.zeros((N, R)), be.zeros((R,)), be.zeros((N, OP))
    rew, done = be.zeros((N,)), be.zeros((N,), np.uint8)
    met = {k: be.zeros((N,), t) for k, t in METRIC_TYPES.items()}
    M = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    be.lib.env_reset(h, N, be.ptr(state), be.ptr(rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(M), be.stream)
    rc = nat.RewardCfg(5.0, 10.0, 2.0, 0.2, 0.5, 0.1, 4.0, 1.0, 1.25)
    r = np.random.default_rng(2)
    snap = lambda: tuple(be.host(x).tobytes() for x in met.values())
    out = dict(state=[], obs=[], done=[], keys=[])
    want = {k: np.zeros(N, t) for k, t in METRIC_TYPES.items()}  # the episode bookkeeping as oracle/env_oracle.py:metrics_step advances it
    for t in range(steps):
        act = be.arr((0.3 * r.standard_normal((N, nu))).astype(f32))
        be.lib.env_step(h, N, 1, C.byref(rc), be.ptr(state), be.ptr(rec), be.ptr(act), nu, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(M), be.stream)
        be.sync()
        out["metrics_step"], out["reward_step"], out["done_step"] = snap(), be.host(rew).tobytes(), be.host(done).tobytes()
        want = metrics_step(want, be.host(rew), be.host(done), f32)
        key = jaxrng.split(KEY, steps)[t]
        s, o = _reinit(be, h, dims, N, impl, mask=be.host(done).copy(), state=state, obs=obs, key=key, event=EVENT + t)
        out["metrics_after"], out["reward_after"], out["done_after"] = snap(), be.host(rew).tobytes(), be.host(done).tobytes()
        out["state"].append(s); out["obs"].append(o); out["done"].append(be.host(done).copy()); out["keys"].append(key)
    out["reset_rec"] = be.host(rec).copy()
    out["met"] = {k: be.host(v).copy() for k, v in met.items()}
    out["met_oracle"] = {k: np.asarray(want[k]).astype(t) for k, t in METRIC_TYPES.items()}
    be.lib.model_close(h)
    return out


@pytest.mark.parametrize("impl", [0, 1])
def test_step_then_reinit_is_the_reference_step(be, impl):
    cm = _cm("pro")
    N, steps = 8, 3
    out = _step_and_reinit(be, cm, N, steps, impl)
    q0 = np.asarray(cm.t["qpos0"], f32)
    OP = out["obs"][0].shape[1]
    for t in range(steps):
        assert out["done"][t].all()
        dq, dv = _noise(impl, N, cm, key=out["keys"][t], event=EVENT + t)
        s = out["state"][t]
        assert np.array_equal(_bits(s[:, :cm.nq]), _bits((q0[None] + dq).astype(f32))) and np.array_equal(_bits(s[:, cm.nq:cm.nq + cm.nv]), _bits(dv))
        assert np.array_equal(_bits(out["obs"][t]), _bits(s[:, :OP]))
        assert not np.array_equal(s, np.tile(out["reset_rec"], (N, 1)))
        if t:
            assert not np.array_equal(s[:, :cm.nq], out["state"][t - 1][:, :cm.nq])  # another step, another draw
    assert out["metrics_after"] == out["metrics_step"]
    for k in METRIC_TYPES:  # all six fields are the step kernel's: the oracle's metrics_step on the steps' own reward / done, float32 like the kernel
        assert np.array_equal(_bits(out["met"][k]), _bits(out["met_oracle"][k])), k
    assert (out["met"]["timestep"] == steps).all() and (out["met"]["returned_episode_lengths"] == 1).all() and (out["met"]["episode_lengths"] == 0).all()


# ---- 7: the engine ----------------------------------------------------------------------------------------------------------------------------------

ENGINE = ["training.num_envs=32", "training.num_steps=3", "rl.num_env_steps=3", "training.num_minibatches=2", "training.update_epochs=1", "model.hidden_size=32",
          "training.total_timesteps=100000", f"environment.reset_noise_scale={S}"]
ALWAYS_DONE = ["reward.height_min_z=5.0", "reward.height_max_z=10.0"]


def _arena(tr, names=("params", "adam_m", "adam_v", "count", "state", "episode_returns", "episode_lengths", "returned_episode", "jax_rng")):
    tr._sync()
    return {n: tr._to_host(tr.region(n)).copy() for n in names}


def _runner_key(seed):
    rng = jaxrng.split(jaxrng.prng_key(seed))[0]
    rng, reset_key = jaxrng.split(rng)
    return jaxrng.split(rng)[1], reset_key


@pytest.mark.parametrize("impl", ["philox", "threefry"])
def test_engine_resets_and_restarts_from_noisy_states(be, impl, tmp_path):
    cfg = make_config(BASE, ENGINE + [f"training.rng_impl={impl}"])
    tr = be.trainer(cfg)
    cm, N, T = tr.cm, tr.N, tr.T
    nq, nv, R, OP = cm.nq, cm.nv, int(tr.dims.rec_dim), tr.OP
    tr.reset()
    tr._sync()
    state = tr._to_host(tr.region("state", (N, R))).copy()
    q0 = np.asarray(cm.t["qpos0"], f32)
    runner, reset_key = _runner_key(tr.seed)
    dq, dv = _noise(1, N, cm, key=reset_key) if impl == "threefry" else _noise(0, N, cm, event=0, seed=tr.seed, rank=0)
    assert np.array_equal(_bits(state[:, :nq]), _bits((q0[None] + dq).astype(f32))) and np.array_equal(_bits(state[:, nq:nq + nv]), _bits(dv))
    assert len({state[n].tobytes() for n in range(N)}) == N and np.abs(dq).max() <= S and np.abs(dv).max() <= S  # (within s of qpos0: the rows ARE qpos0 + dq)
    assert np.array_equal(_bits(tr._to_host(tr.region("obs", (T + 1, N, OP))[0])), _bits(state[:, :OP]))
    # the region reset_rec is the noise-free record: what a trainer at scale 0 holds there, and in every state row
    tr0 = be.trainer(make_config(BASE, [x for x in ENGINE if "reset_noise" not in x] + [f"training.rng_impl={impl}"]))
    tr0.reset()
    tr0._sync()
    assert np.array_equal(_bits(tr._to_host(tr.region("reset_rec"))), _bits(tr0._to_host(tr0.region("reset_rec"))))
    assert np.array_equal(_bits(tr0._to_host(tr0.region("state", (N, R)))), _bits(np.tile(tr0._to_host(tr0.region("reset_rec")), (N, 1))))
    tr0.close()
    # same seed, same bits after three updates; a checkpoint after update 2 resumes to the same bits at update 4
    ck = str(tmp_path / "ck.npz")
    for u in range(4):
        tr.update()
        if u == 1:
            tr.save_checkpoint(ck)
        if u == 2:
            a3 = _arena(tr)
    a4 = _arena(tr)
    assert tr.graph_active() == (be.name == "hip")  # (the device's trainer replays the captured update, masked launches included)
    tr.close()
    b = be.trainer(cfg)
    b.reset()
    for _ in range(3):
        b.update()
    b3 = _arena(b)
    b.close()
    for k in a3:
        assert np.array_equal(_bits(a3[k]), _bits(b3[k])), k
    assert np.isfinite(a3["params"]).all()
    c = be.trainer(cfg)
    c.load_checkpoint(ck)
    for _ in range(2):
        c.update()
    c4 = _arena(c)
    c.close()
    for k in a4:
        assert np.array_equal(_bits(a4[k]), _bits(c4[k])), k
    if be.name == "hip":  # graph replay equals eager launches
        e = be.trainer(cfg, use_graph=False)
        e.reset()
        for _ in range(3):
            e.update()
        assert not e.graph_active()
        e3 = _arena(e)
        e.close()
        for k in a3:
            assert np.array_equal(_bits(a3[k]), _bits(e3[k])), k


@pytest.mark.parametrize("impl", ["philox", "threefry"])
def test_engine_restarts_match_the_restatement_step_by_step(be, impl):
    """Every episode ends at every step (the reward window lies above the robot): observation slots 1 .. T of an update are the noisy restarts of that
    step's key (threefry: the step keys of train.py:163) or event (philox: update * T + 1 + t), in two consecutive updates."""
    cfg = make_config(BASE, ENGINE + ALWAYS_DONE + [f"training.rng_impl={impl}"])
    tr = be.trainer(cfg)
    cm, N, T, OP = tr.cm, tr.N, tr.T, tr.OP
    nq, nv = cm.nq, cm.nv
    q0 = np.asarray(cm.t["qpos0"], f32)
    tr.reset()
    runner, _ = _runner_key(tr.seed)
    seen = []
    for u in range(2):
        tr.update()
        tr._sync()
        obs = tr._to_host(tr.region("obs", (T + 1, N, OP))).copy()
        assert tr._to_host(tr.region("done", (T, N))).all()
        if impl == "threefry":
            runner, _, _, step_keys = jaxrng.update_keys_step(runner, T, tr.E, N * T)
        for t in range(T):
            dq, dv = _noise(1, N, cm, key=step_keys[t]) if impl == "threefry" else _noise(0, N, cm, event=u * T + 1 + t, seed=tr.seed, rank=0)
            assert np.array_equal(_bits(obs[t + 1][:, :nq]), _bits((q0[None] + dq).astype(f32))), (u, t)
            assert np.array_equal(_bits(obs[t + 1][:, nq:nq + nv]), _bits(dv)), (u, t)
            seen.append(obs[t + 1][:, :nq].tobytes())
        state = tr._to_host(tr.region("state", (N, int(tr.dims.rec_dim))))
        assert np.array_equal(_bits(state[:, :OP]), _bits(obs[T]))
    assert len(set(seen)) == 2 * T  # no step repeats another's draw
    tr.close()


# ---- 8: the surface -----------------------------------------------------------------------------------------------------------------------------------


def test_config_key_parses_and_refuses_a_negative_scale():
    assert make_config(BASE).environment.reset_noise_scale == 0.0
    assert make_config(BASE, ["environment.reset_noise_scale=1e-2"]).environment.reset_noise_scale == pytest.approx(0.01)
    assert make_config({**BASE, "environment": {"reset_noise_scale": 0.02}}).environment.reset_noise_scale == pytest.approx(0.02)
    with pytest.raises(ValueError, match="reset_noise_scale"):
        make_config(BASE, ["environment.reset_noise_scale=-0.01"])


def test_set_reset_noise_after_prepare_is_an_error(be):
    cfg = make_config(BASE, [x for x in ENGINE if "reset_noise" not in x])
    tr = be.trainer(cfg)
    assert be.lib._fn["mppo_engine_set_reset_noise"](tr._engine, -1.0) != 0 and "negative" in be.lib.last_error()
    be.lib.engine_set_reset_noise(tr._engine, S)
    be.lib.engine_set_reset_noise(tr._engine, 0.0)
    tr.reset()
    # after the reset the environments hold noise-free initial states: another scale is refused, the one the reset ran with is not
    assert be.lib._fn["mppo_engine_set_reset_noise"](tr._engine, S) != 0 and "mppo_engine_reset has run" in be.lib.last_error()
    be.lib.engine_set_reset_noise(tr._engine, 0.0)
    tr.lib.engine_prepare(tr._engine, tr._stream_ptr)
    tr._sync()
    assert be.lib._fn["mppo_engine_set_reset_noise"](tr._engine, S) != 0
    assert "mppo_engine_set_reset_noise" in be.lib.last_error() and "prepared" in be.lib.last_error()
    with pytest.raises(nat.NativeError):
        be.lib.engine_set_reset_noise(tr._engine, S)
    tr.close()


def test_reinit_refuses_bad_arguments(be):
    cm = _cm("pro")
    h, dims, keep = be.model(cm)
    state = be.zeros((4, dims.rec_dim))
    f = be.lib._fn["mppo_env_reinit"]
    assert f(h, 4, be.ptr(state), 0, 0, 0, -0.5, 0, 1, 0, 0, 0, 0, be.stream) != 0 and "negative" in be.lib.last_error()
    assert f(h, 4, be.ptr(state), 0, 0, 0, S, 1, 1, 0, 0, 0, 0, be.stream) != 0 and "key" in be.lib.last_error()
    assert f(h, 4, be.ptr(state), 0, 0, 0, S, 7, 1, 0, 0, 0, 0, be.stream) != 0 and "rng_impl" in be.lib.last_error()
    assert f(h, 0, be.ptr(state), 0, 0, 0, S, 0, 1, 0, 0, 0, 0, be.stream) != 0
    be.lib.model_close(h)


@pytest.mark.gpu
def test_humanoid_env_draws_the_reference_noise():
    import torch

    from minppo_amd.env import HumanoidEnv

    env = HumanoidEnv(make_config(BASE, [f"environment.reset_noise_scale={S}", "reward.height_min_z=5.0", "reward.height_max_z=10.0"]))
    assert env.reset_noise_scale == pytest.approx(S)
    cm, N = env.cm, 5
    nq, nv = cm.nq, cm.nv
    q0 = np.asarray(cm.t["qpos0"], f32)
    es = env.reset(rng=7, num_envs=N)
    dq, dv = jaxrng.reset_noise(jaxrng.prng_key(7), N, nq, nv, S)
    rec = es.pipeline_state.cpu().numpy()
    assert np.array_equal(_bits(rec[:, :nq]), _bits((q0[None] + dq).astype(f32))) and np.array_equal(_bits(rec[:, nq:nq + nv]), _bits(dv))
    assert np.array_equal(_bits(es.obs.cpu().numpy()), _bits(rec[:, :env.observation_size]))
    es_k = env.reset(rng=jaxrng.prng_key(7), num_envs=N)
    assert torch.equal(es_k.pipeline_state, es.pipeline_state)
    with pytest.raises(ValueError, match="rng"):
        env.reset(rng=None, num_envs=N)
    with pytest.raises(ValueError, match="rng"):
        env.step(es, torch.zeros(N, env.action_size, device=env.device))
    # a step under one key, and under the per-environment keys split from it (train.py:164-165): every episode ends, every environment restarts noisy
    act = torch.zeros(N, env.action_size, device=env.device)
    step_key = np.array([5, 6], np.uint32)
    e1 = env.step(es, act, step_key)
    e2 = env.step(es, act, jaxrng.split(step_key, N))
    assert e1.done.all() and torch.equal(e1.pipeline_state, e2.pipeline_state) and torch.equal(e1.obs, e2.obs)
    dq, dv = jaxrng.reset_noise(step_key, N, nq, nv, S)
    rec = e1.pipeline_state.cpu().numpy()
    assert np.array_equal(_bits(rec[:, :nq]), _bits((q0[None] + dq).astype(f32))) and np.array_equal(_bits(rec[:, nq:nq + nv]), _bits(dv))
    assert (e1.metrics.returned_episode_lengths.cpu().numpy() == 1).all()
    env.close()
    # scale 0: reset / step return what they return today, whatever `rng` is; a directly assigned attribute wins over the config
    plain = HumanoidEnv(make_config(BASE))
    assert plain.reset_noise_scale == 0.0
    a, b = plain.reset(num_envs=N), plain.reset(rng=7, num_envs=N)
    assert torch.equal(a.pipeline_state, b.pipeline_state) and torch.equal(a.obs, b.obs)
    assert torch.equal(a.pipeline_state, plain._reset_rec[None].expand(N, -1))
    act = 0.3 * torch.ones(N, plain.action_size, device=plain.device)
    s1, s2 = plain.step(a, act), plain.step(a, act, np.array([1, 2], np.uint32))
    assert torch.equal(s1.pipeline_state, s2.pipeline_state) and torch.equal(s1.reward, s2.reward)
    plain.reset_noise_scale = 0.02
    c = plain.reset(rng=7, num_envs=N)
    assert float((c.pipeline_state[:, :nq] - plain.initial_qpos[None]).abs().max()) > 0.01
    plain.close()
