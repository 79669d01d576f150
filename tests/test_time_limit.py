"""The episode time limit: the truncation kernel (csrc/k_limit.hip `mppo_env_time_limit`), GAE's cut (`mppo_gae_truncated`), the engine
(`mppo_engine_set_time_limit`), the evaluator (`mppo_evaluate_limit`) and the Python surface (`environment.episode_length`, `HumanoidEnv.step`).

1. the kernel on hand-made arrays, against the NumPy statement of the rule         5. the engine: the rollout is the composition, graph = eager, checkpoint /
2. the staggered first limit, against `jaxrng.time_limit_first_philox`                resume, rollout_stats, off is off, call order
3. GAE: float64 restatement and the exact properties                               6. the evaluator: the composition, L = 0, the counts
4. env steps against `EnvOracle` wrapped with the limit                            7. config keys, HumanoidEnv, the command line

Sizes: N = 37 for the kernel (three workgroups of 16 environments - ten waves of four, the last with one; 16-lane rows), N = 300 for the stagger and GAE (two GAE workgroups), N = 9
for the physics, the smallest engine tests/test_engine.py uses (8 environments, 4 steps)."""

import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from minppo_amd import _native as nat
from minppo_amd import jaxrng
from minppo_amd.config import make_config
from minppo_amd.model import load_model
from minppo_amd.train import init_flat_params, reward_cfg
from oracle import ppo_oracle as po
from oracle.env_oracle import EnvOracle, RewardCfg
from physics_harness import METRIC_TYPES, pack

f32, f64 = np.float32, np.float64
ROOT = Path(__file__).resolve().parent.parent
BASE = {"kscale_id": "5eb3cb7f23232298", "visualization": {"camera_name": "track"}}
SEED = 5
_CM = {}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _cm():
    if "pro" not in _CM:
        _CM["pro"] = load_model("synth_stompy_pro")
    return _CM["pro"]


def _lcfg(length, stagger=0, rank=0, seed=SEED):
    return nat.TimeLimitCfg(length=length, stagger=stagger, rank=rank, reserved=0, seed=seed)


def ref_limit(met, done, L, first=None):
    """The rule in NumPy: -> (truncated, metrics after, done after).  `first`: the staggered first lengths (None: stagger off)."""
    m = {k: np.array(v) for k, v in met.items()}
    ended = np.asarray(done) != 0
    trunc = ~ended & (m["episode_lengths"] >= L)
    if first is not None:
        trunc |= ~ended & (m["timestep"] == m["episode_lengths"]) & (m["episode_lengths"] == first)
    m["returned_episode_returns"][trunc] = m["episode_returns"][trunc]
    m["returned_episode_lengths"][trunc] = m["episode_lengths"][trunc]
    m["returned_episode"][trunc] = 1
    m["episode_returns"][trunc] = 0
    m["episode_lengths"][trunc] = 0
    return trunc, m, (ended | trunc).astype(np.uint8)


# ---- 1: the kernel on hand-made arrays ------------------------------------------------------------------------------------------------------------------


def _hand_made(N, dims, rng):
    R, OP = dims.rec_dim, dims.obs_pad
    lengths = np.array([0, 4, 5, 6], np.int32)[rng.integers(0, 4, N)]
    lengths[:8] = [5, 4, 6, 0, 5, 6, 4, 5]  # (every kind in the first workgroup, whatever the draw)
    done = (rng.random(N) < 0.25).astype(np.uint8)
    done[[0, 5]] = 1   # at the limit with `done` set already: the step ended it, not the limit
    done[[1, 2, 4]] = 0
    met = dict(episode_returns=rng.standard_normal(N).astype(f32), episode_lengths=lengths, returned_episode_returns=rng.standard_normal(N).astype(f32),
               returned_episode_lengths=rng.integers(1, 50, N).astype(np.int32), timestep=rng.integers(100, 200, N).astype(np.int32),
               returned_episode=(rng.random(N) < 0.5).astype(np.uint8))
    return dict(state=rng.standard_normal((N, R)).astype(f32), rec=rng.standard_normal(R).astype(f32), obs=rng.standard_normal((N, OP + 4)).astype(f32), done=done, met=met,
                reward=rng.standard_normal(N).astype(f32))


def _run_limit(be, h, N, cfg, x, with_obs=True, obs_ld=None):
    dims_ld = x["obs"].shape[1] if obs_ld is None else obs_ld
    d = {k: be.arr(x[k]) for k in ("state", "rec", "obs", "done")}
    met = {k: be.arr(v) for k, v in x["met"].items()}
    trunc = be.full((N,), 0xEE, np.uint8)
    Ms = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    be.lib.env_time_limit(h, N, C.byref(cfg), be.ptr(d["state"]), be.ptr(d["rec"]), be.ptr(d["obs"]) if with_obs else 0, dims_ld, be.ptr(d["done"]), be.ptr(trunc),
                          C.byref(Ms), be.stream)
    be.sync()
    return dict(state=be.host(d["state"]).copy(), rec=be.host(d["rec"]).copy(), obs=be.host(d["obs"]).copy(), done=be.host(d["done"]).copy(),
                truncated=be.host(trunc).copy(), met={k: be.host(v).copy() for k, v in met.items()})


def test_kernel_truncates_what_the_rule_says_and_nothing_else(be):
    N, L = 37, 5
    h, dims, _keep = be.model(_cm())
    R, OP = dims.rec_dim, dims.obs_pad
    x = _hand_made(N, dims, np.random.default_rng(0))
    want_t, want_m, want_d = ref_limit(x["met"], x["done"], L)
    assert want_t[[2, 4]].all() and not want_t[[0, 1, 3, 5, 6]].any() and want_t[16:32].any() and want_t[32:].any() and (~want_t[32:]).any()  # lengths 5 and 6; waves with and without a truncated environment
    per_wave = np.add.reduceat(want_t.astype(int), np.arange(0, N, 4))
    assert (per_wave == 0).any() and (per_wave > 0).any() and want_t[36] != want_t[35]  # (the last wave holds one environment)
    got = _run_limit(be, h, N, _lcfg(L), x)
    assert np.array_equal(got["truncated"], want_t.astype(np.uint8)) and np.array_equal(got["done"], want_d)
    for k in METRIC_TYPES:
        assert np.array_equal(_bits(got["met"][k]), _bits(want_m[k])), k
    assert np.array_equal(got["met"]["timestep"], x["met"]["timestep"])
    # the truncated rows are the reset record's bits - the whole record, the observation's pad columns included - and the words behind obs_pad stay
    assert np.array_equal(_bits(got["state"][want_t]), _bits(np.tile(x["rec"], (int(want_t.sum()), 1))))
    assert np.array_equal(_bits(got["obs"][want_t, :OP]), _bits(np.tile(x["rec"][:OP], (int(want_t.sum()), 1))))
    assert np.array_equal(_bits(got["obs"][:, OP:]), _bits(x["obs"][:, OP:]))
    # every other word is what it was
    assert np.array_equal(_bits(got["state"][~want_t]), _bits(x["state"][~want_t])) and np.array_equal(_bits(got["obs"][~want_t]), _bits(x["obs"][~want_t]))
    assert np.array_equal(_bits(got["rec"]), _bits(x["rec"]))
    # obs = NULL: everything else the same
    nul = _run_limit(be, h, N, _lcfg(L), x, with_obs=False)
    assert np.array_equal(_bits(nul["obs"]), _bits(x["obs"])) and np.array_equal(_bits(nul["state"]), _bits(got["state"]))
    assert np.array_equal(nul["truncated"], got["truncated"]) and all(np.array_equal(_bits(nul["met"][k]), _bits(got["met"][k])) for k in METRIC_TYPES)
    # a limit nobody has reached: only the truncated bytes are written
    none = _run_limit(be, h, N, _lcfg(7), x)
    assert not none["truncated"].any() and np.array_equal(_bits(none["state"]), _bits(x["state"])) and np.array_equal(none["done"], x["done"])
    assert all(np.array_equal(_bits(none["met"][k]), _bits(x["met"][k])) for k in METRIC_TYPES)
    # N = 1 and a seed / rank that the unstaggered rule does not read
    one = {k: (v[:1].copy() if k != "rec" and k != "met" else v) for k, v in x.items()}
    one["met"] = {k: v[2:3].copy() for k, v in x["met"].items()}
    one["done"] = x["done"][2:3].copy()
    assert _run_limit(be, h, 1, _lcfg(L, rank=7, seed=99), one)["truncated"][0] == 1
    be.lib.model_close(h)


def test_kernel_refuses_bad_configurations(be):
    N = 8
    h, dims, _keep = be.model(_cm())
    x = _hand_made(N, dims, np.random.default_rng(1))
    d = {k: be.arr(x[k]) for k in ("state", "rec", "obs", "done")}
    met = {k: be.arr(v) for k, v in x["met"].items()}
    trunc = be.zeros((N,), np.uint8)
    Ms = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    f = be.lib._fn["mppo_env_time_limit"]
    ld = x["obs"].shape[1]

    def call(cfg, obs_ld=ld, ms=Ms, n=N):
        return f(h, n, C.byref(cfg), be.ptr(d["state"]), be.ptr(d["rec"]), be.ptr(d["obs"]), obs_ld, be.ptr(d["done"]), be.ptr(trunc), C.byref(ms), be.stream)

    for bad, word in ((_lcfg(-1), "negative"), (_lcfg(0), "no limit"), (_lcfg(5, rank=256), "rank"), (_lcfg(5, rank=-1), "rank")):
        assert call(bad) == -1 and word in be.lib.last_error(), (word, be.lib.last_error())
    assert call(_lcfg(5), obs_ld=dims.obs_pad - 1) == -1 and "obs_ld" in be.lib.last_error()
    assert call(_lcfg(5), n=0) == -1
    no_ts = nat.EnvMetrics(**{k: (0 if k == "timestep" else be.ptr(v)) for k, v in met.items()})
    assert call(_lcfg(5, stagger=1), ms=no_ts) == -1 and "timestep" in be.lib.last_error()
    assert call(_lcfg(5), ms=no_ts) == 0  # (the unstaggered rule does not read it)
    be.sync()
    be.lib.model_close(h)
    with pytest.raises(ValueError):
        jaxrng.time_limit_first_philox(SEED, 0, 4, 0)


# ---- 2: the staggered first limit -----------------------------------------------------------------------------------------------------------------------


def _drive_counters(be, h, dims, N, L, cfg, steps):
    """The kernel on counters alone - no physics: every step adds one to episode_lengths and timestep of every environment -> truncated [steps, N]."""
    state, rec, done = be.zeros((N, dims.rec_dim)), be.zeros((dims.rec_dim,)), be.zeros((N,), np.uint8)
    met = {k: be.zeros((N,), t) for k, t in METRIC_TYPES.items()}
    trunc = be.zeros((N,), np.uint8)
    Ms = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    rows = []
    for _ in range(steps):
        be.put(met["episode_lengths"], be.host(met["episode_lengths"]) + 1)
        be.put(met["timestep"], be.host(met["timestep"]) + 1)
        be.put(done, np.zeros(N, np.uint8))
        be.lib.env_time_limit(h, N, C.byref(cfg), be.ptr(state), be.ptr(rec), 0, dims.obs_pad, be.ptr(done), be.ptr(trunc), C.byref(Ms), be.stream)
        be.sync()
        rows.append(be.host(trunc).copy())
        assert np.array_equal(be.host(done), rows[-1])
    return np.stack(rows) != 0


def test_stagger_shortens_the_first_episode_only(be):
    N, L = 300, 7
    steps = 2 * L + 1
    h, dims, _keep = be.model(_cm())
    firsts = {}
    for rank in (0, 1):
        first = jaxrng.time_limit_first_philox(SEED, rank, N, L)
        firsts[rank] = first
        assert first.min() >= 1 and first.max() <= L and len(set(first.tolist())) == L  # (300 draws of 7 values: every one occurs)
        got = _drive_counters(be, h, dims, N, L, _lcfg(L, stagger=1, rank=rank), steps)
        s = np.arange(1, steps + 1)[:, None]
        want = (s >= first[None]) & ((s - first[None]) % L == 0)  # at first_n, then every L steps
        assert np.array_equal(got, want), rank
        assert (got.sum(0) >= 2).all()
    assert not np.array_equal(firsts[0], firsts[1])
    assert not np.array_equal(jaxrng.time_limit_first_philox(SEED + 1, 0, N, L), firsts[0])
    # stagger off: everybody at L, 2 L, ...
    got = _drive_counters(be, h, dims, N, L, _lcfg(L, stagger=0), steps)
    assert np.array_equal(got, np.tile(((np.arange(1, steps + 1) % L) == 0)[:, None], (1, N)))
    be.lib.model_close(h)


# ---- 3: GAE ---------------------------------------------------------------------------------------------------------------------------------------------

GT, GN, GAMMA, LAM = 7, 300, 0.99, 0.95


def ref_gae_truncated(done, trunc, value, reward, last_val, gamma, lam):
    """oracle.ppo_oracle.calculate_gae with the cut: at a truncated sample adv = 0, target = value, the carried gae 0."""
    T = value.shape[0]
    adv, tgt = np.zeros_like(value), np.zeros_like(value)
    gae, next_value = np.zeros_like(last_val), last_val
    for t in range(T - 1, -1, -1):
        nd = 1.0 - done[t].astype(value.dtype)
        delta = reward[t] + gamma * next_value * nd - value[t]
        gae = delta + gamma * lam * nd * gae
        gae = np.where(trunc[t], 0.0, gae)
        adv[t] = gae
        tgt[t] = np.where(trunc[t], value[t], gae + value[t])
        next_value = value[t]
    return adv, tgt


def _gae_inputs():
    # 0.1 x standard normal: the magnitude of this environment's rewards per step, at which the project's GAE tolerances are stated
    rng = np.random.default_rng(3)
    rew, val, lv = (0.1 * rng.standard_normal((GT, GN))).astype(f32), (0.1 * rng.standard_normal((GT, GN))).astype(f32), (0.1 * rng.standard_normal(GN)).astype(f32)
    trunc = rng.random((GT, GN)) < 0.15
    done = trunc | (rng.random((GT, GN)) < 0.15)
    trunc[GT - 1, :4] = True; done[GT - 1, :4] = True  # a cut at the last step, at the first, twice in a row
    trunc[0, 4:8] = True; done[0, 4:8] = True
    trunc[2:4, 8] = True; done[2:4, 8] = True
    return rew, val, lv, done, trunc


def _gae_run(be, rew, val, lv, done, trunc, entry="truncated"):
    d = [be.arr(x) for x in (rew, val, done.astype(np.uint8))]
    u = be.arr(trunc.astype(np.uint8)) if trunc is not None else None
    l, adv, tgt = be.arr(lv), be.full((GT, GN), np.nan), be.full((GT, GN), np.nan)
    if entry == "truncated":
        be.lib.gae_truncated(GT, GN, GAMMA, LAM, be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), be.ptr(u), be.ptr(l), be.ptr(adv), be.ptr(tgt), be.stream)
    else:
        be.lib.gae(GT, GN, GAMMA, LAM, be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), be.ptr(l), be.ptr(adv), be.ptr(tgt), be.stream)
    be.sync()
    return be.host(adv).copy(), be.host(tgt).copy()


def test_gae_truncated_follows_the_float64_restatement(be):
    rew, val, lv, done, trunc = _gae_inputs()
    adv, tgt = _gae_run(be, rew, val, lv, done, trunc)
    a64, t64 = ref_gae_truncated(done, trunc, val.astype(f64), rew.astype(f64), lv.astype(f64), GAMMA, LAM)
    print(f"adv err max {np.abs(adv - a64).max():.3e}, target err max {np.abs(tgt - t64).max():.3e}")
    np.testing.assert_allclose(adv, a64, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(tgt, t64, rtol=1e-5, atol=1e-6)
    # the restatement without a cut is the project's GAE oracle
    a0, t0 = ref_gae_truncated(done, np.zeros_like(trunc), val.astype(f64), rew.astype(f64), lv.astype(f64), GAMMA, LAM)
    p0 = po.calculate_gae(done, val.astype(f64), rew.astype(f64), lv.astype(f64), GAMMA, LAM)
    np.testing.assert_allclose(a0, p0[0], rtol=1e-14, atol=1e-15); np.testing.assert_allclose(t0, p0[1], rtol=1e-14, atol=1e-15)
    with pytest.raises(nat.NativeError):
        be.lib.gae_truncated(0, GN, GAMMA, LAM, 0, 0, 0, 0, 0, 0, 0, be.stream)


def test_gae_truncated_exact_properties(be):
    rew, val, lv, done, trunc = _gae_inputs()
    plain = _gae_run(be, rew, val, lv, done, None, entry="plain")
    for u in (None, np.zeros_like(trunc)):  # NULL and all-zero: mppo_gae's bits
        got = _gae_run(be, rew, val, lv, done, u)
        assert np.array_equal(_bits(got[0]), _bits(plain[0])) and np.array_equal(_bits(got[1]), _bits(plain[1]))
    adv, tgt = _gae_run(be, rew, val, lv, done, trunc)
    assert (_bits(adv[trunc]) == 0).all()  # exactly +0
    assert np.array_equal(_bits(tgt[trunc]), _bits(val[trunc]))
    assert not np.array_equal(adv, plain[0])
    # the rewards at and after a truncated step change no bit of the advantages before it
    rng = np.random.default_rng(8)
    first_cut = np.where(trunc.any(0), trunc.argmax(0), GT)  # per environment: the first truncated step (GT: none)
    rew2 = rew.copy()
    at_or_after = np.arange(GT)[:, None] >= first_cut[None]
    rew2[at_or_after] = rng.standard_normal(int(at_or_after.sum())).astype(f32)
    adv2, tgt2 = _gae_run(be, rew2, val, lv, done, trunc)
    before = ~at_or_after
    assert before.any() and (first_cut < GT).sum() > GN // 2
    assert np.array_equal(_bits(adv2[before]), _bits(adv[before])) and np.array_equal(_bits(tgt2[before]), _bits(tgt[before]))
    # ... while without the cut they do (the property is the cut's, not the inputs')
    p2 = _gae_run(be, rew2, val, lv, done, None, entry="plain")
    assert not np.array_equal(p2[0][before], plain[0][before])


# ---- 7a: config -------------------------------------------------------------------------------------------------------------------------------------------


def test_config_keys_defaults_and_refusals():
    env = make_config(BASE).environment
    assert (env.episode_length, env.episode_length_stagger) == (0, True)
    got = make_config(BASE, ["environment.episode_length=1000", "environment.episode_length_stagger=false"]).environment
    assert (got.episode_length, got.episode_length_stagger) == (1000, False)
    with pytest.raises(ValueError, match="episode_length"):
        make_config(BASE, ["environment.episode_length=-1"])


# ---- 4: env steps against the wrapped EnvOracle ---------------------------------------------------------------------------------------------------------


CEILING = {1: 2.2e-4, 2: 5.2e-4}  # height_max_z above the standing height, per n_frames: in a gap of the oracle's heights (the test prints and asserts the margin)


class LimitedEnvOracle:
    """oracle.env_oracle.EnvOracle with the time limit behind its step, in float64 (Brax: EpisodeWrapper around the environment): an environment whose
    episode did not end and whose post-step length has reached L is truncated - done, the returned_* metrics, zeroed running metrics, the reset state
    and the reset observation, exactly what the step does for an ended episode."""

    def __init__(self, env, L):
        self.env, self.L = env, L

    def reset(self, N):
        es = self.env.reset(N)
        es["truncation"] = np.zeros(N, bool)
        return es

    def step(self, es, action):
        env = self.env
        N = action.shape[0]
        out = env.step({k: v for k, v in es.items() if k != "truncation"}, action)
        trunc, m, _ = ref_limit(out["metrics"], out["done"], self.L)
        m["returned_episode"] = m["returned_episode"].astype(bool)
        s_reset = env._get_reset_state(N)
        s = out["pipeline_state"]
        for k, v in list(s.items()):
            if isinstance(v, np.ndarray) and v.shape[:1] == (N,) and k in s_reset:
                s[k] = np.where(trunc.reshape((N,) + (1,) * (v.ndim - 1)), s_reset[k], v)
        out["obs"] = np.where(trunc[:, None], env.get_obs(s_reset), out["obs"])
        out["metrics"], out["done"], out["truncation"] = m, out["done"] | trunc, trunc
        return out


@pytest.mark.parametrize("n_frames", [1, 2])
def test_env_step_and_limit_match_the_wrapped_env_oracle(be, n_frames):
    """The envelope of tests/test_push.py::test_env_step_xfrc_matches_env_oracle (the kernel re-seeded from the oracle state before every step, that test's
    tolerances) with mppo_env_time_limit behind every step.  N = 9, L = 4, 12 steps.  The window's ceiling lies a little above the standing height, as in
    tests/test_evaluate.py, where a gap of the oracle's own heights is: some environments rise through it within four steps (terminations), most do not
    (truncations); no height of the run lies within 1e-5 of it - a hundred float32 roundings of a height of 1 - so the flags are compared exactly."""
    cm = _cm()
    h, dims, _keep = be.model(cm, True)
    N, L, O, OP, R, nv, nu = 9, 4, dims.obs_dim, dims.obs_pad, dims.rec_dim, cm.nv, cm.nu
    z0 = float(np.asarray(cm.t["qpos0"])[2])
    rcfg = RewardCfg(height_min_z=-0.2, height_max_z=z0 + CEILING[n_frames])
    env = LimitedEnvOracle(EnvOracle(cm.t, rcfg, include_c_vals=True, n_frames=n_frames), L)
    state, reset_rec, obs = be.zeros((N, R)), be.zeros((R,)), be.full((N, OP), np.nan)
    rew, done, trunc = be.zeros((N,)), be.zeros((N,), np.uint8), be.zeros((N,), np.uint8)
    met = {k: be.full((N,), 7, dt) for k, dt in METRIC_TYPES.items()}
    Ms = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    be.lib.env_reset(h, N, be.ptr(state), be.ptr(reset_rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(Ms), be.stream)
    es = env.reset(N)
    rc = nat.RewardCfg(rcfg.height_min_z, rcfg.height_max_z, 2.0, 0.2, 0.5, 0.1, 4.0, 1.0, 1.25)
    lc = _lcfg(L)
    rng = np.random.default_rng(1)
    n_term, n_trunc, margin, dv_all = 0, 0, np.inf, []
    for t in range(12):
        a = (0.6 * rng.standard_normal((N, nu))).astype(f32)
        be.put(state, pack(env.env, es["pipeline_state"], dims, nv))
        for k in met:
            be.put(met[k], es["metrics"][k].astype(METRIC_TYPES[k]))
        da = be.arr(a)
        be.lib.env_step(h, N, n_frames, C.byref(rc), be.ptr(state), be.ptr(reset_rec), be.ptr(da), nu, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(Ms), be.stream)
        be.sync()
        z_kernel = be.host(state)[:, 2].copy()
        stepped_done = be.host(done).astype(bool)
        be.lib.env_time_limit(h, N, C.byref(lc), be.ptr(state), be.ptr(reset_rec), be.ptr(obs), OP, be.ptr(done), be.ptr(trunc), C.byref(Ms), be.stream)
        be.sync()
        es = env.step(es, a.astype(f64))
        s = es["pipeline_state"]
        got_done, got_trunc = be.host(done).astype(bool), be.host(trunc).astype(bool)
        live = ~stepped_done  # (an ended environment's row holds the reset height)
        if live.any():
            margin = min(margin, float(np.abs(z_kernel[live] - rcfg.height_max_z).min()))
        assert np.array_equal(got_done, es["done"]), (t, got_done, es["done"])
        assert np.array_equal(got_trunc, es["truncation"]), (t, got_trunc, es["truncation"])
        n_trunc += int(got_trunc.sum()); n_term += int((got_done & ~got_trunc).sum())
        np.testing.assert_allclose(be.host(obs)[:, :O], es["obs"], atol=1e-4)
        np.testing.assert_allclose(be.host(rew), es["reward"], atol=1e-2)
        st = be.host(state)
        np.testing.assert_allclose(st[:, :cm.nq], s.qpos, atol=2e-3 * n_frames)
        dv_all.append(np.abs(st[:, cm.nq:cm.nq + nv] - s.qvel)[~got_done].max(1) if (~got_done).any() else np.zeros(0))
        np.testing.assert_allclose(st[:, OP + nv + 1], s.time, atol=1e-6)
        for k in met:
            g, w = be.host(met[k]), es["metrics"][k]
            if METRIC_TYPES[k] == f32:
                np.testing.assert_allclose(g, w, rtol=1e-4, atol=1e-2)
            else:
                assert (g == w.astype(g.dtype)).all(), (t, k, g, w)
    dv = np.concatenate(dv_all)
    print(f"n_frames {n_frames}: {n_term} terminations, {n_trunc} truncations, the nearest live height {margin:.3e} from the ceiling; dv max {dv.max():.3e} median {np.median(dv):.3e}")
    assert n_term >= 1 and n_trunc >= 2 * N
    assert margin > 1e-5
    assert dv.max() <= 1.0 * n_frames and np.mean(dv > 0.15 * n_frames) <= 0.05 and np.median(dv) <= 0.02 * n_frames
    be.lib.model_close(h)


# ---- 5: the engine --------------------------------------------------------------------------------------------------------------------------------------

NE, TE, LE = 8, 4, 3
ENGINE = [f"training.num_envs={NE}", f"training.num_steps={TE}", f"rl.num_env_steps={TE}", "training.num_minibatches=2", "training.update_epochs=2", "model.hidden_size=32",
          "training.total_timesteps=100000"]  # (the smallest engine of tests/test_engine.py)
LIMITED = [f"environment.episode_length={LE}"]
# (tests/test_obs_norm.py: a window that ends episodes at every step in some environments - terminations beside the truncations - under reset noise)
FALLING = ["environment.reset_noise_scale=0.01", "reward.height_min_z=1.005", "reward.height_max_z=1.012"]
NORMS = ["training.normalize_observations=true", "training.normalize_rewards=true"]


def _host(tr, name, shape=None):
    tr._sync()
    return np.array(tr._to_host(tr.region(name, shape)))


def _write_random(be, tr, rng):
    noise = rng.standard_normal((tr.T, tr.N, tr.A)).astype(f32)
    perms = np.stack([rng.permutation(tr.N * tr.T) for _ in range(tr.E)]).astype(np.int32)
    be.put(tr.region("noise", (tr.T, tr.N, tr.A)), noise)
    be.put(tr.region("perm", (tr.E, tr.N * tr.T)), perms)
    return noise


@pytest.mark.parametrize("extra", [[], FALLING, FALLING + NORMS], ids=["plain", "reset_noise", "reset_noise_and_norms"])
def test_rollout_equals_the_composition_of_the_stages(be, extra):
    """Update 2's rollout written out with the ABI's own stages from the engine's state after update 1: per step mppo_policy_forward, mppo_env_step,
    mppo_env_time_limit (stagger on, the engine's seed and rank), [mppo_env_reinit over done, event T + 1 + t], [mppo_obs_norm_apply]; then the bootstrap
    forward, [mppo_reward_norm_apply], mppo_gae_truncated - bit for bit.  (Noise and permutations are written by the test: external_random.)"""
    cfg = make_config(BASE, ENGINE + LIMITED + extra)
    noisy, normed = bool(extra), len(extra) > len(FALLING)
    tr = be.trainer(cfg, external_random=True)
    assert tr.episode_length == LE
    tr.reset()
    rng = np.random.default_rng(11)
    _write_random(be, tr, rng)
    tr.update()
    N, Tn, O, OP, A = tr.N, tr.T, tr.O, tr.OP, tr.A
    host = lambda name, shape=None: _host(tr, name, shape)
    first = jaxrng.time_limit_first_philox(tr.seed, 0, N, LE)
    tr1 = host("truncated", (Tn, N)) != 0
    # update 1: every environment's first episode is cut at its own first_n (where it did not fall before)
    d1 = host("done", (Tn, N)) != 0
    for n in range(N):
        fell = np.flatnonzero(d1[:, n] & ~tr1[:, n])
        if fell.size == 0 or fell[0] >= first[n] - 1:
            assert tr1[first[n] - 1, n] or (fell.size and fell[0] == first[n] - 1), (n, first[n], tr1[:, n])
    assert (tr1 <= d1).all()
    state, rec, params = be.arr(host("state", (N, tr.dims.rec_dim))), be.arr(host("reset_rec")), be.arr(host("params"))
    obs = be.arr(host("obs", (Tn + 1, N, OP)))
    met = {k: be.arr(host(k).astype(t)) for k, t in METRIC_TYPES.items()}
    on_stats, on_table = host("obs_norm_stats"), host("obs_norm_table", (2, OP))
    rn_stats, rn_table, rn_carry = host("reward_norm_stats"), host("reward_norm_table"), host("reward_norm_carry")
    noise = _write_random(be, tr, rng)
    tr.rollout()
    tr._sync()
    # ---- the replay
    lib, s = be.lib, be.stream
    M = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    noise_d = be.arr(noise)
    act, logp, val, last = be.zeros((Tn, N, A)), be.zeros((Tn, N)), be.zeros((Tn, N)), be.zeros((N,))
    rew, done, trunc = be.zeros((Tn, N)), be.zeros((Tn, N), np.uint8), be.full((Tn, N), 0xEE, np.uint8)
    scaled, adv, target = be.zeros((Tn, N)), be.zeros((Tn, N)), be.zeros((Tn, N))
    wsb = lib.policy_ws_bytes(C.byref(tr.net), N)
    ws = be.zeros((wsb,), np.uint8)
    G, GR = lib.obs_norm_partials(N), lib.reward_norm_partials(N)
    part, sdev, tdev = be.zeros((Tn, G, 2, O), f64), be.arr(on_stats), be.arr(on_table)
    rpart, rsdev, rtdev, rcdev = be.zeros((GR, 2), f64), be.arr(rn_stats), be.arr(rn_table), be.arr(rn_carry)
    rc = reward_cfg(cfg)
    lc = _lcfg(LE, stagger=1, rank=0, seed=int(tr.seed))
    row, arow, prow = N * OP * 4, N * A * 4, G * 2 * O * 8
    gamma, lam = float(f32(cfg.rl.gamma)), float(f32(cfg.rl.gae_lambda))
    for t in range(Tn):
        lib.policy_forward(C.byref(tr.net), be.ptr(params), N, be.ptr(obs) + t * row, OP, be.ptr(noise_d) + t * arow, be.ptr(act) + t * arow, be.ptr(logp) + t * N * 4,
                           be.ptr(val) + t * N * 4, 0, be.ptr(ws), wsb, s)
        lib.env_step(tr._model, N, cfg.environment.n_frames, C.byref(rc), be.ptr(state), be.ptr(rec), be.ptr(act) + t * arow, A, be.ptr(obs) + (t + 1) * row, OP,
                     be.ptr(rew) + t * N * 4, be.ptr(done) + t * N, C.byref(M), s)
        lib.env_time_limit(tr._model, N, C.byref(lc), be.ptr(state), be.ptr(rec), be.ptr(obs) + (t + 1) * row, OP, be.ptr(done) + t * N, be.ptr(trunc) + t * N, C.byref(M), s)
        if noisy:
            lib.env_reinit(tr._model, N, be.ptr(state), be.ptr(obs) + (t + 1) * row, OP, be.ptr(done) + t * N, float(cfg.environment.reset_noise_scale), 0, int(tr.seed), 0,
                           0, 0, Tn + 1 + t, s)
        if normed:
            lib.obs_norm_apply(N, O, be.ptr(obs) + (t + 1) * row, OP, be.ptr(tdev), OP, float(cfg.training.obs_norm_clip), be.ptr(part) + t * prow, s)
    lib.policy_forward(C.byref(tr.net), be.ptr(params), N, be.ptr(obs) + Tn * row, OP, 0, 0, 0, be.ptr(last), 0, be.ptr(ws), wsb, s)
    if normed:
        lib.reward_norm_apply(Tn, N, gamma, be.ptr(rew), be.ptr(done), be.ptr(rcdev), be.ptr(rtdev), float(cfg.training.reward_norm_clip), be.ptr(scaled), be.ptr(rpart), s)
    lib.gae_truncated(Tn, N, gamma, lam, be.ptr(scaled if normed else rew), be.ptr(val), be.ptr(done), be.ptr(trunc), be.ptr(last), be.ptr(adv), be.ptr(target), s)
    be.sync()
    pairs = [("obs", obs), ("action", act), ("reward", rew), ("done", done), ("truncated", trunc), ("value", val), ("last_val", last), ("adv", adv), ("target", target),
             ("state", state)] + [(k, met[k]) for k in METRIC_TYPES]
    if normed:
        pairs += [("reward_scaled", scaled), ("reward_norm_carry", rcdev), ("obs_norm_partials", part)]
    for name, mine in pairs:
        assert np.array_equal(_bits(host(name)).reshape(-1), _bits(be.host(mine)).reshape(-1)), name
    dn, tn = host("done", (Tn, N)) != 0, host("truncated", (Tn, N)) != 0
    print(f"{extra and 'noisy' or 'plain'}: update 2 has {int(tn.sum())} truncations and {int((dn & ~tn).sum())} terminations in {Tn * N} samples")
    assert tn.any() and (tn <= dn).all() and not dn.all()
    if noisy:
        assert (dn & ~tn).any(), "the window must end some episodes beside the truncated ones"
    # what GAE made of the truncated samples, and the statistics: episodes = every done, truncated = the region's count
    assert (_bits(host("adv", (Tn, N))[tn]) == 0).all() and np.array_equal(_bits(host("target", (Tn, N))[tn]), _bits(host("value", (Tn, N))[tn]))
    st = tr.rollout_stats()
    assert st["episodes"] == dn.sum() and st["truncated"] == tn.sum() and host("rollout_stats")[6] == tn.sum()
    assert set(st) == {"mean_reward", "done_fraction", "episodes", "mean_episode_return", "mean_episode_length", "truncated"}
    tr.close()


def _arena(tr, names=("params", "adam_m", "adam_v", "count", "state", "episode_returns", "episode_lengths", "returned_episode")):
    tr._sync()
    return {n: tr._to_host(tr.region(n)).copy() for n in names}


def _run(be, cfg, updates, before=None, names=None, **kw):
    tr = be.trainer(cfg, **kw)
    if before is not None:
        before(tr)
    tr.reset()
    for _ in range(updates):
        tr.update()
    out = _arena(tr) if names is None else _arena(tr, names)
    graph = tr.graph_active()
    stats = tr.rollout_stats()
    tr.close()
    return out, graph, stats


def test_episode_length_zero_is_an_engine_that_never_heard_of_it(be):
    cfg = make_config(BASE, ENGINE)
    never, _, st_never = _run(be, cfg, 3)
    zero, _, st_zero = _run(be, cfg, 3, before=lambda tr: be.lib.engine_set_time_limit(tr._engine, 0, 1))
    keyed, _, _ = _run(be, make_config(BASE, ENGINE + ["environment.episode_length=0", "environment.episode_length_stagger=false"]), 3)
    limited, _, st_lim = _run(be, make_config(BASE, ENGINE + LIMITED), 3)
    for k in never:
        assert np.array_equal(_bits(never[k]), _bits(zero[k])) and np.array_equal(_bits(never[k]), _bits(keyed[k])), k
    assert "truncated" not in st_never and "truncated" not in st_zero and st_never == st_zero
    assert st_never["episodes"] == 0 and st_lim["episodes"] > 0 and st_lim["truncated"] > 0  # the statistics a standing policy no longer produces, and produces again
    assert not np.array_equal(never["episode_lengths"], limited["episode_lengths"]) and np.isfinite(limited["params"]).all()
    # the region is there, and untouched, without a limit
    tr = be.trainer(cfg)
    tr.reset(); tr.update()
    assert _host(tr, "truncated").shape == (TE * NE,) and not _host(tr, "truncated").any() and _host(tr, "rollout_stats")[6] == 0
    tr.close()


def test_limited_engine_graph_checkpoint_and_resume(be, tmp_path):
    """Four updates with a checkpoint after the second (update 2 holds truncations, so do 3 and 4: L = 3, T = 4): resumed = uninterrupted, bit for bit; on the
    device the uninterrupted run replays its captured graph, and three eager updates leave what three replayed ones leave."""
    cfg = make_config(BASE, ENGINE + LIMITED + FALLING)
    names = ("params", "adam_m", "adam_v", "count", "state", "episode_returns", "episode_lengths", "returned_episode", "returned_episode_lengths", "timestep", "truncated",
             "done", "adv")
    ck = str(tmp_path / "ck.npz")
    tr = be.trainer(cfg)
    tr.reset()
    for u in range(4):
        tr.update()
        if u == 1:
            tr.save_checkpoint(ck)
        if u == 2:
            a3 = _arena(tr, names)
            assert a3["truncated"].any()
    a4 = _arena(tr, names)
    assert a4["truncated"].any() and tr.graph_active() == (be.name == "hip")
    tr.close()
    c = be.trainer(cfg)
    c.load_checkpoint(ck)
    for _ in range(2):
        c.update()
    c4 = _arena(c, names)
    c.close()
    for k in a4:
        assert np.array_equal(_bits(a4[k]), _bits(c4[k])), k
    if be.name == "hip":
        e3, graph, _ = _run(be, cfg, 3, names=names, use_graph=False)
        assert not graph
        for k in a3:
            assert np.array_equal(_bits(a3[k]), _bits(e3[k])), k


def test_set_time_limit_call_order_and_refusals(be):
    tr = be.trainer(make_config(BASE, ENGINE))
    f = be.lib._fn["mppo_engine_set_time_limit"]
    assert f(tr._engine, -1, 1) == -1 and "negative" in be.lib.last_error()  # MPPO_EINVAL
    assert f(0, 5, 1) == -1
    be.lib.engine_set_time_limit(tr._engine, 5, 1)
    be.lib.engine_set_time_limit(tr._engine, 0, 0)
    be.lib.engine_set_time_limit(tr._engine, 7, 0)
    tr.reset()
    assert f(tr._engine, 5, 1) == -4 and "mppo_engine_reset has run" in be.lib.last_error()  # MPPO_ESTATE
    tr.lib.engine_prepare(tr._engine, tr._stream_ptr)
    tr._sync()
    assert f(tr._engine, 5, 1) == -4 and "mppo_engine_set_time_limit" in be.lib.last_error() and "prepared" in be.lib.last_error()
    with pytest.raises(nat.NativeError):
        be.lib.engine_set_time_limit(tr._engine, 0, 0)
    tr.close()
    # any number of ranks: the rank enters the stream, nothing crosses ranks
    two = be.trainer(make_config(BASE, ENGINE + LIMITED), world_size=2, rank=1)
    assert two.episode_length == LE
    two.close()


# ---- 6: the evaluator -----------------------------------------------------------------------------------------------------------------------------------

EN, EK, ER, EH, EL = 20, 10, 3, 64, 4
# nobody falls in ten steps / with reset noise 0.01 around the standing height of 1.0095, a floor of 1.005 (tests/test_evaluate.py "deterministic_noise"): the
# environments that start, or restart, below it fall at once, the others stand
STANDING, FALLS = (-0.2, 2.0), (1.005, 2.0)
_EVALS = {}


def _eval_setup(be):
    cm = _cm()
    h, dims, keep = be.model(cm)
    net = nat.Net(dims.obs_dim, dims.obs_pad, dims.nu, EH, 1, 0, 2)
    params = init_flat_params(3, dims.obs_dim, dims.nu, EH)
    return cm, h, dims, keep, net, params


def _ecfg(window, noise=0.0, det=0):
    rc = reward_cfg(make_config(BASE, [f"reward.height_min_z={window[0]}", f"reward.height_max_z={window[1]}"]))
    return nat.EvalCfg(N=EN, K=EK, n_frames=1, deterministic=det, record_envs=ER, reset_noise_scale=noise, seed=SEED, reward=rc)


def _evaluate(be, L, window=STANDING, noise=0.0, entry="limit"):
    """mppo_evaluate_limit (or _push) -> (result bytes, extra bytes, trajectory); once per backend and argument set."""
    key = (be.name, L, window, noise, entry)
    if key in _EVALS:
        return _EVALS[key]
    cm, h, dims, keep, net, params = _eval_setup(be)
    e = _ecfg(window, noise)
    need = (be.lib.eval_limit_ws_bytes if entry == "limit" else be.lib.eval_ws_bytes)(h, C.byref(net), C.byref(e))
    assert need > 0 and be.lib.eval_limit_ws_bytes(h, C.byref(net), C.byref(e)) > be.lib.eval_ws_bytes(h, C.byref(net), C.byref(e))
    ws = be.full((need,), 0xA5, np.uint8)
    res, extra = be.full((C.sizeof(nat.EvalResultRaw) // 8,), -1, np.int64), be.full((2,), -1, np.int64)
    traj = be.full((EK + 1, ER, cm.nq + cm.nv + dims.nu + 2), np.nan)
    p_dev = be.arr(params)
    if entry == "limit":
        be.lib.evaluate_limit(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), need, 0, 0.0, None, L, be.ptr(res), be.ptr(extra), be.ptr(traj), be.stream)
    else:
        be.lib.evaluate_push(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), need, 0, 0.0, None, be.ptr(res), be.ptr(traj), be.stream)
    be.sync()
    out = (be.host(res).tobytes(), be.host(extra).tobytes(), be.host(traj).copy())
    be.lib.model_close(h)
    _EVALS[key] = out
    return out


def _by_hand(be, L, window, noise):
    """The documented sequence of mppo_evaluate_limit written out with the library's entry points."""
    cm, h, dims, keep, net, params = _eval_setup(be)
    e = _ecfg(window, noise)
    lib, s = be.lib, be.stream
    OP, RD, A, nqv = dims.obs_pad, dims.rec_dim, dims.nu, cm.nq + cm.nv
    W = nqv + A + 2
    state, rec, obs = be.zeros((EN, RD)), be.zeros((RD,)), be.zeros((EN, OP))
    rew, done, trunc = be.zeros((EN,)), be.zeros((EN,), np.uint8), be.zeros((EN,), np.uint8)
    met = {k: be.full((EN,), 3, t) for k, t in METRIC_TYPES.items()}
    Ms = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    p_dev = be.arr(params)
    act, logp, val, noise_d = be.zeros((EN, A)), be.zeros((EN,)), be.zeros((EN,)), be.zeros((EN, A))
    wsb = lib.policy_ws_bytes(C.byref(net), EN)
    ws = be.zeros((wsb,), np.uint8)
    acc, lacc = be.full((nat.EVAL_ACC_SLOTS * EN,), -1, np.int64), be.full((2 * EN,), -1, np.int64)
    res, extra = be.full((C.sizeof(nat.EvalResultRaw) // 8,), -1, np.int64), be.full((2,), -1, np.int64)
    lc = _lcfg(L, stagger=0, rank=0, seed=SEED)
    lib.env_reset(h, EN, be.ptr(state), be.ptr(rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(Ms), s)
    if noise > 0:
        lib.env_reinit(h, EN, be.ptr(state), be.ptr(obs), OP, 0, noise, 0, SEED, 0, 0, 0, 0, s)
    be.sync()
    frame0 = np.zeros((ER, W), f32)
    frame0[:, :nqv] = be.host(state)[:ER, :nqv]
    rows, flags = [frame0], []
    for t in range(EK):
        lib.normal_fill(SEED, t, EN * A, be.ptr(noise_d), s)
        lib.policy_forward(C.byref(net), be.ptr(p_dev), EN, be.ptr(obs), OP, be.ptr(noise_d), be.ptr(act), be.ptr(logp), be.ptr(val), 0, be.ptr(ws), wsb, s)
        lib.env_step(h, EN, e.n_frames, C.byref(e.reward), be.ptr(state), be.ptr(rec), be.ptr(act), A, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(Ms), s)
        lib.env_time_limit(h, EN, C.byref(lc), be.ptr(state), be.ptr(rec), be.ptr(obs), OP, be.ptr(done), be.ptr(trunc), C.byref(Ms), s)
        if noise > 0:
            lib.env_reinit(h, EN, be.ptr(state), be.ptr(obs), OP, be.ptr(done), noise, 0, SEED, 0, 0, 0, t + 1, s)
        row = be.zeros((ER, W))
        lib.eval_accumulate(EN, int(t == 0), be.ptr(rew), be.ptr(done), C.byref(Ms), be.ptr(acc), be.ptr(state), RD, nqv, be.ptr(act), A, A, ER, be.ptr(row), s)
        lib.eval_limit_count(EN, int(t == 0), be.ptr(done), be.ptr(trunc), be.ptr(lacc), s)
        be.sync()
        rows.append(be.host(row).copy())
        flags.append((be.host(done).astype(bool), be.host(trunc).astype(bool)))
    lib.eval_limit_reduce(EN, be.ptr(lacc), be.ptr(extra), s)
    lib.eval_reduce(EN, EK, be.ptr(acc), be.ptr(res), s)
    be.sync()
    out = (be.host(res).tobytes(), be.host(extra).tobytes(), np.stack(rows), flags)
    lib.model_close(h)
    return out


@pytest.mark.parametrize("window,noise", [(STANDING, 0.0), (FALLS, 0.01)], ids=["standing", "falls_and_reset_noise"])
def test_evaluate_limit_is_the_composition(be, window, noise):
    raw, extra, traj = _evaluate(be, EL, window, noise)
    raw_h, extra_h, traj_h, flags = _by_hand(be, EL, window, noise)
    assert not np.isnan(traj).any()
    assert np.array_equal(_bits(traj), _bits(traj_h)) and raw == raw_h and extra == extra_h
    dn, tn = np.stack([f[0] for f in flags]), np.stack([f[1] for f in flags])
    r, x = nat.EvalResultRaw.from_buffer_copy(raw), nat.EvalLimitResultRaw.from_buffer_copy(extra)
    fallen = int((dn & ~tn).any(0).sum())
    print(f"window {window}: {int(tn.sum())} truncated episodes, {int((dn & ~tn).sum())} falls in {fallen} environments")
    assert (x.truncated_episodes, x.fallen_envs) == (int(tn.sum()), fallen) and r.episodes == int(dn.sum())
    assert np.array_equal(traj[1:, :, -1] != 0, dn[:, :ER])  # the trajectory's done column includes the truncations
    if window == STANDING:
        assert x.truncated_episodes == 2 * EN and x.fallen_envs == 0 and r.len_min == r.len_max == EL and r.survivors == 0
    else:
        assert 0 < fallen < EN and x.truncated_episodes > 0


def test_evaluate_limit_with_length_zero_is_evaluate_push(be):
    plain = _evaluate(be, 0, FALLS, 0.01, entry="push")
    zero = _evaluate(be, 0, FALLS, 0.01)
    assert zero[0] == plain[0] and np.array_equal(_bits(zero[2]), _bits(plain[2]))
    assert zero[1] == np.full(2, -1, np.int64).tobytes()  # *extra is not written
    limited = _evaluate(be, EL, FALLS, 0.01)
    assert limited[0] != plain[0]
    # refusals
    cm, h, dims, keep, net, params = _eval_setup(be)
    e = _ecfg(STANDING)
    need = be.lib.eval_limit_ws_bytes(h, C.byref(net), C.byref(e))
    ws, res, p_dev = be.zeros((need,), np.uint8), be.zeros((14,), np.int64), be.arr(params)
    traj = be.zeros((EK + 1, ER, cm.nq + cm.nv + dims.nu + 2))
    f = be.lib._fn["mppo_evaluate_limit"]
    assert f(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), need, 0, 0.0, None, -1, be.ptr(res), be.ptr(res) + 96, be.ptr(traj), be.stream) == -1
    assert "negative" in be.lib.last_error()
    assert f(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), need, 0, 0.0, None, 4, be.ptr(res), 0, be.ptr(traj), be.stream) == -1
    small = be.lib.eval_ws_bytes(h, C.byref(net), C.byref(e))
    assert f(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), small, 0, 0.0, None, 4, be.ptr(res), be.ptr(res) + 96, be.ptr(traj), be.stream) != 0
    assert "mppo_eval_limit_ws_bytes" in be.lib.last_error()
    be.lib.model_close(h)


@pytest.mark.parametrize("window,noise", [(STANDING, 0.0), (FALLS, 0.01)], ids=["standing", "falls"])
def test_python_evaluate_counts_the_environments_that_never_fell(be, window, noise):
    from minppo_amd.evaluate import evaluate

    raw, extra, traj = _evaluate(be, EL, window, noise)
    r, x = nat.EvalResultRaw.from_buffer_copy(raw), nat.EvalLimitResultRaw.from_buffer_copy(extra)
    cfg = make_config(BASE, [f"model.hidden_size={EH}", f"training.seed={SEED}", f"evaluation.num_envs={EN}", f"evaluation.num_steps={EK}", f"evaluation.record_envs={ER}",
                             "evaluation.deterministic=false", f"environment.episode_length={EL}", f"environment.reset_noise_scale={noise}",
                             f"reward.height_min_z={window[0]}", f"reward.height_max_z={window[1]}"])
    cm = _cm()
    flat = init_flat_params(3, cm.obs_size(True), cm.nu, EH)
    device = {} if be.name == "emu" else {"device": "cuda:0"}
    got = evaluate(cfg, flat, lib=be.lib, xp=be.xp, **device)
    assert got.episodes == r.episodes and got.truncated_episodes == x.truncated_episodes and got.falls == r.episodes - x.truncated_episodes
    assert got.survivors == EN - x.fallen_envs and np.isnan(got.survivor_mean_return)
    assert np.array_equal(_bits(got.trajectory["qpos"]), _bits(traj[..., :cm.nq]))
    st = got.stats()
    assert {"truncated_episodes", "falls"} <= set(st) and len(st) == 14
    if window == STANDING:
        assert (got.truncated_episodes, got.falls, got.survivors) == (2 * EN, 0, EN)
    else:
        assert 0 < got.survivors < EN and got.falls >= EN - got.survivors
    # without a limit the key set and the meaning of `survivors` are what they were
    plain = evaluate(make_config(BASE, [f"model.hidden_size={EH}", f"evaluation.num_envs={EN}", "evaluation.num_steps=2"]), flat, lib=be.lib, xp=be.xp, **device)
    assert set(plain.stats()) == {"episodes", "mean_return", "std_return", "min_return", "max_return", "mean_length", "min_length", "max_length", "survivors",
                                  "survivor_mean_return", "mean_reward", "steps"} and plain.truncated_episodes is None


# ---- 7: the host surface --------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
def test_humanoid_env_reports_truncation():
    import torch

    from minppo_amd.env import HumanoidEnv

    L, N = 3, 5
    env = HumanoidEnv(make_config(BASE, [f"environment.episode_length={L}"]))
    es = env.reset(num_envs=N)
    assert es.truncation is None  # (the reset truncates nothing)
    act = 0.1 * torch.ones(N, env.action_size, device=env.device)
    reset_state = es.pipeline_state.clone()
    for t in range(2 * L):
        es = env.step(es, act)
        cut = (t + 1) % L == 0
        assert es.truncation.dtype == torch.bool and es.truncation.shape == (N,)
        assert bool(es.truncation.all()) == cut and bool(es.truncation.any()) == cut and bool(es.done.all()) == cut
        if cut:
            assert torch.equal(es.pipeline_state, reset_state) and int(es.metrics.returned_episode_lengths[0]) == L and int(es.metrics.episode_lengths[0]) == 0
            assert torch.equal(es.obs, reset_state[:, :env.observation_size])
    assert int(es.metrics.timestep[0]) == 2 * L
    env.close()
    plain = HumanoidEnv(make_config(BASE))
    e1 = plain.step(plain.reset(num_envs=N), act)
    assert e1.truncation is None and len(e1) == 6
    plain.close()


@pytest.mark.gpu
def test_train_and_evaluate_under_a_time_limit_from_the_command_line(tmp_path):
    model = str(tmp_path / "model.pkl")
    small = ["training.num_envs=64", "training.num_minibatches=2", "model.hidden_size=64", "environment.episode_length=8"]
    p = subprocess.run([sys.executable, "-m", "minppo_amd.cli", "train", "stompy_pro", *small, "training.total_timesteps=1280", f"training.model_save_path={model}"],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert p.returncode == 0 and Path(model).exists(), p.stderr[-2000:]
    p = subprocess.run([sys.executable, "-m", "minppo_amd.cli", "evaluate", "stompy_pro", *small, "evaluation.num_envs=20", "evaluation.num_steps=8",
                        f"inference.model_path={model}"], capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1
    out = json.loads(line[0])
    assert set(out) == {"episodes", "mean_return", "std_return", "min_return", "max_return", "mean_length", "min_length", "max_length", "survivors",
                        "survivor_mean_return", "mean_reward", "steps", "truncated_episodes", "falls"}
    assert out["steps"] == 160 and out["episodes"] > 0 and out["truncated_episodes"] + out["falls"] == out["episodes"] and out["survivor_mean_return"] is None
