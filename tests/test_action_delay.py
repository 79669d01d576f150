"""Actuation latency: the latency table and the delay stage (csrc/k_sensor.hip `mppo_action_delay_fill` / `_apply`) against the semantic rule, and - together with
the sensor noise of tests/test_obs_noise.py - the engine (`mppo_engine_set_obs_noise` / `_set_action_delay`) and the evaluator (`mppo_evaluate_sensors`) against
their compositions written out with the library's own stage entry points.  Every comparison is bit for bit.

The rule: at the k-th step of an episode environment n is given the policy's action of step k - d_n of the same episode, zeros while k < d_n, the very bits of the
policy's action when d_n = 0.

Sizes: D = 1, 3, 16 with N = 1, 5, 67 and A = 10 (the robots') or 7 (odd, with act_ld > A) for the stage; the smallest engine tests/test_time_limit.py uses
(8 environments, 4 steps) and its evaluation (20 environments, 10 steps, 3 recorded)."""

import ctypes as C

import numpy as np
import pytest

from minppo_amd import _native as nat
from minppo_amd import jaxrng
from minppo_amd.config import make_config
from minppo_amd.model import load_model
from minppo_amd.train import init_flat_params, obs_noise_scales, reward_cfg
from physics_harness import METRIC_TYPES

f32, f64 = np.float32, np.float64
BASE = {"kscale_id": "5eb3cb7f23232298", "visualization": {"camera_name": "track"}}
SEED = 5
_CM = {}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _cm():
    if "pro" not in _CM:
        _CM["pro"] = load_model("synth_stompy_pro")
    return _CM["pro"]


def _dcfg(dmin, dmax, rank=0, seed=SEED):
    return nat.ActionDelayCfg(min=dmin, max=dmax, rank=rank, reserved=0, seed=seed)


def rule(actions, done_before, delays):
    """The semantic rule in NumPy.  actions [S][N][A] the policy's; done_before[s][n]: environment n restarted right before step s (its episode step is 0 there);
    -> applied [S][N][A]."""
    S, N, A = actions.shape
    out = np.zeros_like(actions)
    k = np.zeros(N, np.int64)
    for s in range(S):
        k[done_before[s]] = 0
        for n in range(N):
            d = int(delays[n])
            if d == 0:
                out[s, n] = actions[s, n]
            elif k[n] >= d:
                out[s, n] = actions[s - d, n]
        k += 1
    return out


# ---- the table ----------------------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("N", [1, 5, 67])
def test_latency_table_equals_the_restatement(be, N):
    for dmin, dmax, rank, seed in ((0, 16, 0, SEED), (0, 3, 0, SEED), (2, 2, 0, SEED), (0, 0, 0, SEED), (1, 16, 7, SEED), (3, 5, 255, 2**63 + 11)):
        d = be.full((N + 3,), -7, np.int32)
        be.lib.action_delay_fill(C.byref(_dcfg(dmin, dmax, rank, seed)), N, be.ptr(d), be.stream)
        be.sync()
        got = be.host(d)
        want = jaxrng.action_delays_philox(seed, rank, N, dmin, dmax)
        assert want.dtype == np.int32 and np.array_equal(got[:N], want) and (got[N:] == -7).all(), (dmin, dmax, rank)
        assert want.min() >= dmin and want.max() <= dmax
        if dmin == dmax:
            assert (want == dmin).all()
    if N == 67:  # every latency of 0 .. 3 is drawn, and 17 values over 67 environments are spread
        assert set(jaxrng.action_delays_philox(SEED, 0, N, 0, 3)) == {0, 1, 2, 3} and len(set(jaxrng.action_delays_philox(SEED, 0, N, 0, 16))) > 12


def test_delay_stage_refusals(be):
    N, A = 5, 10
    d, ts, ep = be.zeros((N,), np.int32), be.zeros((N,), np.int32), be.zeros((N,), np.int32)
    act, hist, app = be.zeros((N, A)), be.zeros((3, N, A)), be.zeros((N, A))
    f, g = be.lib._fn["mppo_action_delay_fill"], be.lib._fn["mppo_action_delay_apply"]
    for cfg, word in ((_dcfg(-1, 2), "-1"), (_dcfg(3, 2), "3"), (_dcfg(0, 17), "17"), (_dcfg(0, 2, rank=256), "256"), (_dcfg(0, 2, rank=-1), "-1")):
        assert f(C.byref(cfg), N, be.ptr(d), be.stream) == -1 and word in be.lib.last_error(), word
        assert g(C.byref(cfg), N, A, be.ptr(d), be.ptr(ts), be.ptr(ep), be.ptr(act), A, be.ptr(hist), be.ptr(app), A, be.stream) == -1
    assert f(None, N, be.ptr(d), be.stream) == -1 and f(C.byref(_dcfg(0, 2)), N, 0, be.stream) == -1 and f(C.byref(_dcfg(0, 2)), 0, be.ptr(d), be.stream) == -1
    ok = _dcfg(0, 3)
    args = lambda **kw: [kw.get(k, v) for k, v in (("cfg", C.byref(ok)), ("N", N), ("A", A), ("d", be.ptr(d)), ("ts", be.ptr(ts)), ("ep", be.ptr(ep)), ("act", be.ptr(act)),
                                                    ("ld", A), ("hist", be.ptr(hist)), ("app", be.ptr(app)), ("ald", A), ("s", be.stream))]
    assert g(*args()) == 0
    for k in ("d", "ts", "ep", "act", "hist", "app"):
        assert g(*args(**{k: 0})) == -1 and "null" in be.lib.last_error(), k
    assert g(*args(ld=A - 1)) == -1 and g(*args(ald=A - 1)) == -1 and "act_ld" in be.lib.last_error()
    assert g(*args(cfg=C.byref(_dcfg(0, 0)))) == -1 and "nothing to launch" in be.lib.last_error()
    assert g(*args(N=0)) == -1 and g(*args(A=0)) == -1
    be.sync()


# ---- the stage on a scripted run ---------------------------------------------------------------------------------------------------------------------------------


def _scripted(be, D, N, A, act_ld, app_ld, delays, start=0):
    """3 D + 2 steps of counter actions a[s][n][i] = s + n / 128 + i / 1024 under hand-placed `done` flags, the metrics kept as the environment kernel keeps them
    (timestep counts every step since the reset, episode_lengths restarts behind a done) -> (policy actions, applied actions, restarts, final ring)."""
    S = 3 * D + 2
    s_, n_, i_ = np.meshgrid(np.arange(S), np.arange(N), np.arange(A), indexing="ij")
    a = (s_ + n_ / 128 + i_ / 1024).astype(f32)
    assert np.array_equal(a.astype(f64), s_ + n_ / 128 + i_ / 1024)  # (exact in float32: every value names its step, environment and column)
    a[1, :, 0] = -0.0  # (a sign bit the d = 0 rows must hand on)
    sn, nn = np.meshgrid(np.arange(S), np.arange(N), indexing="ij")
    done = ((sn * 5 + nn * 3) % 11 == 0) | ((sn == D) & (nn % 2 == 0)) | ((sn == D + 1) & (nn % 4 == 0)) | ((sn == 2 * D) & (nn % 3 == 1))  # done[s][n]: step s ended n's episode
    ddev, ts, ep = be.arr(np.asarray(delays, np.int32)), be.full((N,), start, np.int32), be.zeros((N,), np.int32)
    hist = be.zeros((D, N, A))
    act, app = be.full((N, act_ld), np.nan), be.full((N, app_ld), np.nan)
    cfg = _dcfg(0, D)
    got = np.zeros((S, N, A), f32)
    ts_h, ep_h = np.full(N, start, np.int32), np.zeros(N, np.int32)
    for s in range(S):
        row = np.full((N, act_ld), np.nan, f32)
        row[:, :A] = a[s]
        be.put(act, row)
        be.lib.action_delay_apply(C.byref(cfg), N, A, be.ptr(ddev), be.ptr(ts), be.ptr(ep), be.ptr(act), act_ld, be.ptr(hist), be.ptr(app), app_ld, be.stream)
        be.sync()
        out = be.host(app)
        assert np.isnan(out[:, A:]).all()  # (the columns behind A are not written)
        got[s] = out[:, :A]
        ts_h, ep_h = ts_h + 1, np.where(done[s], 0, ep_h + 1).astype(np.int32)
        be.put(ts, ts_h)
        be.put(ep, ep_h)
    before = np.concatenate([np.zeros((1, N), bool), done[:-1]])
    return a, got, before, be.host(hist).copy()


@pytest.mark.parametrize("D", [1, 3, 16])
@pytest.mark.parametrize("N,A,act_ld,app_ld", [(1, 10, 10, 10), (5, 7, 9, 8), (67, 10, 10, 10), (67, 7, 12, 7)])
def test_delay_stage_obeys_the_rule_on_a_scripted_run(be, D, N, A, act_ld, app_ld):
    tables = [(D - np.arange(N)) % (D + 1)]  # environment 0 waits the full D, environment D does not wait
    if N == 67:
        tables.append(jaxrng.action_delays_philox(SEED, 0, N, 0, D))
    for delays in tables:
        for start in (0, 2**31 - 1 - (3 * D + 2) if N == 5 else 5):  # (the ring's index is the timestep's remainder, whatever it started from)
            a, got, before, hist = _scripted(be, D, N, A, act_ld, app_ld, delays, start)
            want = rule(a, before, delays)
            assert np.array_equal(_bits(got), _bits(want)), (D, N, A, start)
            S = a.shape[0]
            for n in range(N):
                d = int(delays[n])
                starts = [0] + [s for s in range(1, S) if before[s, n]]
                for s0 in starts:  # zeros on the first d steps of every episode (as far as the episode and the run go), nothing from before a restart
                    nxt = min([s for s in starts if s > s0] + [S])
                    assert not got[s0:min(s0 + d, nxt), n].any()
                if d == 0:
                    assert np.array_equal(_bits(got[:, n]), _bits(a[:, n])) and np.signbit(got[1, n, 0])
            assert before[1:].any()
            # the ring holds the last D actions, by timestep
            for s in range(S - D, S):
                assert np.array_equal(_bits(hist[(start + s) % D]), _bits(a[s]))


# ---- the engine is the composition --------------------------------------------------------------------------------------------------------------------------------

NE, TE, LE = 8, 4, 3
ENGINE = [f"training.num_envs={NE}", f"training.num_steps={TE}", f"rl.num_env_steps={TE}", "training.num_minibatches=2", "training.update_epochs=2", "model.hidden_size=32",
          "training.total_timesteps=100000"]
# (tests/test_time_limit.py: a limit of three steps, and a window that ends episodes at every step in some environments, under reset noise)
HARD = [f"environment.episode_length={LE}", "environment.reset_noise_scale=0.01", "reward.height_min_z=1.005", "reward.height_max_z=1.012", "training.normalize_observations=true"]
DMIN, DMAX = 0, 2
SENSORS = ["environment.obs_noise_level=0.05", "environment.obs_noise_cinert=0.5", f"environment.action_delay_min={DMIN}", f"environment.action_delay_max={DMAX}"]


def _host(tr, name, shape=None):
    tr._sync()
    return np.array(tr._to_host(tr.region(name, shape)))


def test_rollout_equals_the_composition_of_the_stages(be):
    """Update 2's rollout written out with the ABI's own stages from the engine's state after update 1: per step mppo_policy_forward, mppo_action_delay_apply,
    mppo_env_step on the applied action, mppo_env_time_limit, mppo_env_reinit over done, mppo_obs_noise_apply at the explicit step T + t + 1, mppo_obs_norm_apply;
    then the bootstrap forward and mppo_gae_truncated - bit for bit.  (Noise and permutations are written by the test: external_random.)"""
    cfg = make_config(BASE, ENGINE + HARD + SENSORS)
    tr = be.trainer(cfg, external_random=True)
    tr.reset()
    rng = np.random.default_rng(11)

    def write_random():
        noise = rng.standard_normal((tr.T, tr.N, tr.A)).astype(f32)
        be.put(tr.region("noise", (tr.T, tr.N, tr.A)), noise)
        be.put(tr.region("perm", (tr.E, tr.N * tr.T)), np.stack([rng.permutation(tr.N * tr.T) for _ in range(tr.E)]).astype(np.int32))
        return noise

    N, Tn, O, OP, A = tr.N, tr.T, tr.O, tr.OP, tr.A
    host = lambda name, shape=None: _host(tr, name, shape)
    sigma = obs_noise_scales(cfg, _cm())
    delays = jaxrng.action_delays_philox(tr.seed, 0, N, DMIN, DMAX)
    assert np.array_equal(host("action_delay"), delays) and set(delays) == {0, 1, 2} and np.array_equal(host("obs_noise_scale")[:O], sigma) and not host("obs_noise_scale")[O:].any()
    # the reset's row: the exact observation (the state record's leading words) plus the noise of step 0
    live = sigma > 0
    exact0 = host("state", (N, tr.dims.rec_dim))[:, :O]
    obs0 = host("obs", (Tn + 1, N, OP))[0]
    assert np.array_equal(_bits(obs0[:, :O][:, live]), _bits((exact0 + jaxrng.obs_noise_philox(tr.seed, 0, 0, N, sigma))[:, live]))
    assert np.array_equal(_bits(obs0[:, :O][:, ~live]), _bits(exact0[:, ~live])) and not obs0[:, O:].any()
    write_random()
    tr.update()
    state, rec, params = be.arr(host("state", (N, tr.dims.rec_dim))), be.arr(host("reset_rec")), be.arr(host("params"))
    obs = be.arr(host("obs", (Tn + 1, N, OP)))
    met = {k: be.arr(host(k).astype(t)) for k, t in METRIC_TYPES.items()}
    on_table = host("obs_norm_table", (2, OP))
    hist = be.arr(host("action_hist", (16, N, A))[:DMAX])
    assert not host("action_hist", (16, N, A))[DMAX:].any()
    noise = write_random()
    tr.rollout()
    tr._sync()
    # ---- the replay
    lib, s = be.lib, be.stream
    M = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    noise_d = be.arr(noise)
    act, logp, val, last = be.zeros((Tn, N, A)), be.zeros((Tn, N)), be.zeros((Tn, N)), be.zeros((N,))
    applied, app_all = be.zeros((N, A)), []
    rew, done, trunc = be.zeros((Tn, N)), be.zeros((Tn, N), np.uint8), be.full((Tn, N), 0xEE, np.uint8)
    adv, target = be.zeros((Tn, N)), be.zeros((Tn, N))
    wsb = lib.policy_ws_bytes(C.byref(tr.net), N)
    ws = be.zeros((wsb,), np.uint8)
    G = lib.obs_norm_partials(N)
    part, tdev = be.zeros((Tn, G, 2, O), f64), be.arr(on_table)
    sig_table = np.zeros(OP, f32)
    sig_table[:O] = sigma
    sdev, ddev = be.arr(sig_table), be.arr(delays)
    rc = reward_cfg(cfg)
    lc = nat.TimeLimitCfg(length=LE, stagger=1, rank=0, reserved=0, seed=int(tr.seed))
    nc, dc = nat.ObsNoiseCfg(seed=int(tr.seed), rank=0, reserved=0), _dcfg(DMIN, DMAX, 0, int(tr.seed))
    row, arow, prow = N * OP * 4, N * A * 4, G * 2 * O * 8
    gamma, lam = float(f32(cfg.rl.gamma)), float(f32(cfg.rl.gae_lambda))
    ep_before = []
    for t in range(Tn):
        lib.policy_forward(C.byref(tr.net), be.ptr(params), N, be.ptr(obs) + t * row, OP, be.ptr(noise_d) + t * arow, be.ptr(act) + t * arow, be.ptr(logp) + t * N * 4,
                           be.ptr(val) + t * N * 4, 0, be.ptr(ws), wsb, s)
        be.sync()
        ep_before.append(be.host(met["episode_lengths"]).copy())
        lib.action_delay_apply(C.byref(dc), N, A, be.ptr(ddev), be.ptr(met["timestep"]), be.ptr(met["episode_lengths"]), be.ptr(act) + t * arow, A, be.ptr(hist),
                               be.ptr(applied), A, s)
        lib.env_step(tr._model, N, cfg.environment.n_frames, C.byref(rc), be.ptr(state), be.ptr(rec), be.ptr(applied), A, be.ptr(obs) + (t + 1) * row, OP,
                     be.ptr(rew) + t * N * 4, be.ptr(done) + t * N, C.byref(M), s)
        lib.env_time_limit(tr._model, N, C.byref(lc), be.ptr(state), be.ptr(rec), be.ptr(obs) + (t + 1) * row, OP, be.ptr(done) + t * N, be.ptr(trunc) + t * N, C.byref(M), s)
        lib.env_reinit(tr._model, N, be.ptr(state), be.ptr(obs) + (t + 1) * row, OP, be.ptr(done) + t * N, float(cfg.environment.reset_noise_scale), 0, int(tr.seed), 0,
                       0, 0, Tn + 1 + t, s)
        lib.obs_noise_apply(C.byref(nc), N, O, be.ptr(obs) + (t + 1) * row, OP, be.ptr(sdev), 0, 0, Tn + t + 1, s)
        lib.obs_norm_apply(N, O, be.ptr(obs) + (t + 1) * row, OP, be.ptr(tdev), OP, float(cfg.training.obs_norm_clip), be.ptr(part) + t * prow, s)
        be.sync()
        app_all.append(be.host(applied).copy())
    lib.policy_forward(C.byref(tr.net), be.ptr(params), N, be.ptr(obs) + Tn * row, OP, 0, 0, 0, be.ptr(last), 0, be.ptr(ws), wsb, s)
    lib.gae_truncated(Tn, N, gamma, lam, be.ptr(rew), be.ptr(val), be.ptr(done), be.ptr(trunc), be.ptr(last), be.ptr(adv), be.ptr(target), s)
    be.sync()
    pairs = [("obs", obs), ("action", act), ("action_applied", applied), ("reward", rew), ("done", done), ("truncated", trunc), ("value", val), ("last_val", last),
             ("adv", adv), ("target", target), ("state", state), ("log_prob", logp), ("obs_norm_partials", part)] + [(k, met[k]) for k in METRIC_TYPES]
    for name, mine in pairs:
        assert np.array_equal(_bits(host(name)).reshape(-1), _bits(be.host(mine)).reshape(-1)), name
    assert np.array_equal(_bits(host("action_hist", (16, N, A))[:DMAX]), _bits(be.host(hist)))
    # at least one environment restarted inside the run, and every environment with a latency was given zeros right behind its restart
    dn = be.host(done) != 0
    acts, app_all = be.host(act), np.stack(app_all)
    assert dn[:-1].any() and not dn.all()
    seen = 0
    for t in range(Tn):
        for n in range(N):
            d, k = int(delays[n]), int(ep_before[t][n])
            if d > 0 and k < d:
                assert not app_all[t, n].any()
                seen += int(t > 0 and dn[t - 1, n])
            elif d > 0 and t - d >= 0:
                assert np.array_equal(_bits(app_all[t, n]), _bits(acts[t - d, n]))
            elif d == 0:
                assert np.array_equal(_bits(app_all[t, n]), _bits(acts[t, n]))
    assert seen > 0, "no environment with a latency restarted inside the rollout"
    tr.close()


_NAMES = ("params", "adam_m", "adam_v", "count", "state", "episode_returns", "episode_lengths", "returned_episode", "returned_episode_lengths", "timestep", "truncated", "done",
          "adv", "target", "obs", "action", "action_applied", "action_hist", "reward", "value")


def _arena(tr):
    tr._sync()
    return {n: tr._to_host(tr.region(n)).copy() for n in _NAMES}


def test_sensor_engine_graph_checkpoint_and_resume(be, tmp_path):
    """Four updates with a checkpoint after the second: resumed = uninterrupted, bit for bit (the ring of past actions travels in the checkpoint, the noise's step
    follows the device's update counter); on the device the uninterrupted run replays its captured graph, and three eager updates leave what three replayed ones leave."""
    cfg = make_config(BASE, ENGINE + HARD + SENSORS)
    ck = str(tmp_path / "ck.npz")
    tr = be.trainer(cfg)
    tr.reset()
    for u in range(4):
        tr.update()
        if u == 1:
            tr.save_checkpoint(ck)
        if u == 2:
            a3 = _arena(tr)
    a4 = _arena(tr)
    assert a4["done"].any() and a4["action_hist"].any() and tr.graph_active() == (be.name == "hip")
    tr.close()
    with np.load(ck) as z:
        assert "action_hist" in z.files and z["action_hist"].any()
    c = be.trainer(cfg)
    c.load_checkpoint(ck)
    for _ in range(2):
        c.update()
    c4 = _arena(c)
    c.close()
    for k in a4:
        assert np.array_equal(_bits(a4[k]), _bits(c4[k])), k
    # a run with another noise or another latency does not continue this checkpoint
    for other in (["environment.obs_noise_level=0.1"], ["environment.action_delay_max=3"], ["environment.obs_noise_level=0"]):
        o = be.trainer(make_config(BASE, ENGINE + HARD + SENSORS + other))
        with pytest.raises(ValueError, match="obs_noise|action_delay"):
            o.load_checkpoint(ck)
        o.close()
    if be.name == "hip":
        e = be.trainer(cfg, use_graph=False)
        e.reset()
        for _ in range(3):
            e.update()
        e3 = _arena(e)
        assert not e.graph_active()
        e.close()
        for k in a3:
            assert np.array_equal(_bits(a3[k]), _bits(e3[k])), k


# ---- the evaluator ------------------------------------------------------------------------------------------------------------------------------------------------

EN, EK, ER, EH, EL = 20, 10, 3, 64, 4
FALLS = (1.005, 2.0)  # (tests/test_time_limit.py: with reset noise 0.01 around the standing height the environments that start, or restart, below the floor fall at once)
ENOISE = 0.01


def _eval_setup(be):
    cm = _cm()
    h, dims, keep = be.model(cm)
    net = nat.Net(dims.obs_dim, dims.obs_pad, dims.nu, EH, 1, 0, 2)
    params = init_flat_params(3, dims.obs_dim, dims.nu, EH)
    return cm, h, dims, keep, net, params


def _ecfg(det=0):
    rc = reward_cfg(make_config(BASE, [f"reward.height_min_z={FALLS[0]}", f"reward.height_max_z={FALLS[1]}"]))
    return nat.EvalCfg(N=EN, K=EK, n_frames=1, deterministic=det, record_envs=ER, reset_noise_scale=ENOISE, seed=SEED, reward=rc)


def _esigma():
    return obs_noise_scales(make_config(BASE, ["environment.obs_noise_level=0.05"]), _cm())


def _evaluate(be, entry, sigma=None, delay=None, det=0):
    cm, h, dims, keep, net, params = _eval_setup(be)
    e = _ecfg(det)
    need = (be.lib.eval_sensors_ws_bytes if entry == "sensors" else be.lib.eval_domain_ws_bytes)(h, C.byref(net), C.byref(e))
    assert be.lib.eval_sensors_ws_bytes(h, C.byref(net), C.byref(e)) > be.lib.eval_domain_ws_bytes(h, C.byref(net), C.byref(e)) > 0
    ws = be.full((need,), 0xA5, np.uint8)
    res, extra = be.full((C.sizeof(nat.EvalResultRaw) // 8,), -1, np.int64), be.full((2,), -1, np.int64)
    traj, tapp = be.full((EK + 1, ER, cm.nq + cm.nv + dims.nu + 2), np.nan), be.full((EK + 1, ER, dims.nu), np.nan)
    p_dev = be.arr(params)
    if entry == "sensors":
        be.lib.evaluate_sensors(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), need, 0, 0.0, None, EL, None, None if sigma is None else sigma.ctypes.data,
                                None if delay is None else C.byref(delay), be.ptr(res), be.ptr(extra), be.ptr(traj), be.ptr(tapp), be.stream)
    else:
        be.lib.evaluate_domain(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), need, 0, 0.0, None, EL, None, be.ptr(res), be.ptr(extra), be.ptr(traj), be.stream)
    be.sync()
    out = (be.host(res).tobytes(), be.host(extra).tobytes(), be.host(traj).copy(), be.host(tapp).copy())
    be.lib.model_close(h)
    return out


def _by_hand(be, sigma, delay, det=0):
    """The documented sequence of mppo_evaluate_sensors written out with the library's entry points."""
    cm, h, dims, keep, net, params = _eval_setup(be)
    e = _ecfg(det)
    lib, s = be.lib, be.stream
    O, OP, RD, A, nqv = dims.obs_dim, dims.obs_pad, dims.rec_dim, dims.nu, cm.nq + cm.nv
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
    lc = nat.TimeLimitCfg(length=EL, stagger=0, rank=0, reserved=0, seed=SEED)
    nc = nat.ObsNoiseCfg(seed=SEED, rank=0, reserved=0)
    table = np.zeros(OP, f32)
    table[:O] = sigma
    sdev = be.arr(table)
    dc = _dcfg(delay.min, delay.max, 0, SEED)
    ddev, hist, applied = be.zeros((EN,), np.int32), be.zeros((delay.max, EN, A)), be.zeros((EN, A))
    lib.env_reset(h, EN, be.ptr(state), be.ptr(rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(Ms), s)
    lib.env_reinit(h, EN, be.ptr(state), be.ptr(obs), OP, 0, ENOISE, 0, SEED, 0, 0, 0, 0, s)
    lib.obs_noise_apply(C.byref(nc), EN, O, be.ptr(obs), OP, be.ptr(sdev), 0, 0, 0, s)
    lib.action_delay_fill(C.byref(dc), EN, be.ptr(ddev), s)
    be.sync()
    frame0 = np.zeros((ER, W), f32)
    frame0[:, :nqv] = be.host(state)[:ER, :nqv]
    rows, arows, flags, eps = [frame0], [np.zeros((ER, A), f32)], [], []
    for t in range(EK):
        if not det:
            lib.normal_fill(SEED, t, EN * A, be.ptr(noise_d), s)
        lib.policy_forward(C.byref(net), be.ptr(p_dev), EN, be.ptr(obs), OP, be.ptr(noise_d), be.ptr(act), be.ptr(logp), be.ptr(val), 0, be.ptr(ws), wsb, s)
        be.sync()
        eps.append(be.host(met["episode_lengths"]).copy())
        lib.action_delay_apply(C.byref(dc), EN, A, be.ptr(ddev), be.ptr(met["timestep"]), be.ptr(met["episode_lengths"]), be.ptr(act), A, be.ptr(hist), be.ptr(applied), A, s)
        lib.env_step(h, EN, e.n_frames, C.byref(e.reward), be.ptr(state), be.ptr(rec), be.ptr(applied), A, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(Ms), s)
        lib.env_time_limit(h, EN, C.byref(lc), be.ptr(state), be.ptr(rec), be.ptr(obs), OP, be.ptr(done), be.ptr(trunc), C.byref(Ms), s)
        lib.env_reinit(h, EN, be.ptr(state), be.ptr(obs), OP, be.ptr(done), ENOISE, 0, SEED, 0, 0, 0, t + 1, s)
        lib.obs_noise_apply(C.byref(nc), EN, O, be.ptr(obs), OP, be.ptr(sdev), 0, 0, t + 1, s)
        row = be.zeros((ER, W))
        lib.eval_accumulate(EN, int(t == 0), be.ptr(rew), be.ptr(done), C.byref(Ms), be.ptr(acc), be.ptr(state), RD, nqv, be.ptr(act), A, A, ER, be.ptr(row), s)
        lib.eval_limit_count(EN, int(t == 0), be.ptr(done), be.ptr(trunc), be.ptr(lacc), s)
        be.sync()
        rows.append(be.host(row).copy())
        arows.append(be.host(applied)[:ER].copy())
        flags.append(be.host(done).astype(bool))
    lib.eval_limit_reduce(EN, be.ptr(lacc), be.ptr(extra), s)
    lib.eval_reduce(EN, EK, be.ptr(acc), be.ptr(res), s)
    be.sync()
    out = (be.host(res).tobytes(), be.host(extra).tobytes(), np.stack(rows), np.stack(arows), np.stack(flags), np.stack(eps), be.host(ddev).copy())
    lib.model_close(h)
    return out


@pytest.mark.parametrize("det", [0, 1], ids=["sampled", "deterministic"])
def test_evaluate_sensors_is_the_composition(be, det):
    sigma, delay = _esigma(), _dcfg(0, 3, rank=99, seed=123)  # (rank and seed of the configuration are not read: rank 0, the evaluation's seed)
    raw, extra, traj, tapp = _evaluate(be, "sensors", sigma, delay, det)
    raw_h, extra_h, traj_h, tapp_h, dn, eps, delays = _by_hand(be, sigma, delay, det)
    assert not np.isnan(traj).any() and not np.isnan(tapp).any()
    assert np.array_equal(_bits(traj), _bits(traj_h)) and np.array_equal(_bits(tapp), _bits(tapp_h)) and raw == raw_h and extra == extra_h
    assert np.array_equal(delays, jaxrng.action_delays_philox(SEED, 0, EN, 0, 3)) and len(set(delays[:ER])) > 1
    # the recorded applied action obeys the rule; the trajectory's action columns are the policy's
    A = tapp.shape[2]
    act = traj[1:, :, -A - 2:-2]
    before = np.concatenate([np.zeros((1, ER), bool), dn[:-1, :ER]])
    assert np.array_equal(_bits(tapp[1:]), _bits(rule(act, before, delays[:ER]))) and not tapp[0].any()
    assert dn[:-1, :ER].any(), "a recorded environment must restart inside the run"
    for t in range(EK):
        for n in range(ER):
            if eps[t][n] < delays[n]:
                assert not tapp[t + 1, n].any()
    # noise and latency change the evaluation, under the mean action too
    plain = _evaluate(be, "domain", det=det)
    assert plain[0] != raw


def test_evaluate_sensors_with_both_options_off_is_evaluate_domain(be):
    plain = _evaluate(be, "domain")
    for sigma, delay in ((None, None), (np.zeros(225, f32), _dcfg(0, 0)), (None, _dcfg(0, 0, rank=300))):
        off = _evaluate(be, "sensors", sigma, delay)
        assert off[0] == plain[0] and off[1] == plain[1] and np.array_equal(_bits(off[2]), _bits(plain[2]))
        assert np.isnan(off[3]).all()  # the applied actions' trajectory is written only under a latency
    # refusals at the C boundary: a negative sigma (the vector is the host's here), the latency's range, the workspace
    cm, h, dims, keep, net, params = _eval_setup(be)
    e = _ecfg()
    need = be.lib.eval_sensors_ws_bytes(h, C.byref(net), C.byref(e))
    ws, res, p_dev = be.zeros((need,), np.uint8), be.zeros((14,), np.int64), be.arr(params)
    traj = be.zeros((EK + 1, ER, cm.nq + cm.nv + dims.nu + 2))
    f = be.lib._fn["mppo_evaluate_sensors"]
    call = lambda sig, dl, nbytes=need: f(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), nbytes, 0, 0.0, None, EL, None, sig, dl, be.ptr(res), be.ptr(res) + 96,
                                           be.ptr(traj), 0, be.stream)
    bad = _esigma()
    bad[3] = -1.0
    assert call(bad.ctypes.data, None) == -1 and "column 3" in be.lib.last_error() and "negative" in be.lib.last_error()
    assert call(None, C.byref(_dcfg(2, 1))) == -1 and call(None, C.byref(_dcfg(0, 17))) == -1 and "17" in be.lib.last_error()
    assert call(None, C.byref(_dcfg(-1, 1))) == -1
    assert call(None, None, be.lib.eval_domain_ws_bytes(h, C.byref(net), C.byref(e))) != 0 and "mppo_eval_sensors_ws_bytes" in be.lib.last_error()
    assert call(None, C.byref(_dcfg(0, 2))) == 0  # (no trajectory of applied actions asked for: NULL)
    be.sync()
    be.lib.model_close(h)


@pytest.mark.parametrize("det", [False, True], ids=["sampled", "deterministic"])
def test_python_evaluate_goes_through_the_sensors(be, det):
    from minppo_amd.evaluate import evaluate

    raw, extra, traj, tapp = _evaluate(be, "sensors", _esigma(), _dcfg(0, 3), int(det))
    r = nat.EvalResultRaw.from_buffer_copy(raw)
    cfg = make_config(BASE, [f"model.hidden_size={EH}", f"training.seed={SEED}", f"evaluation.num_envs={EN}", f"evaluation.num_steps={EK}", f"evaluation.record_envs={ER}",
                             f"evaluation.deterministic={str(det).lower()}", f"environment.episode_length={EL}", f"environment.reset_noise_scale={ENOISE}",
                             f"reward.height_min_z={FALLS[0]}", f"reward.height_max_z={FALLS[1]}", "environment.obs_noise_level=0.05", "environment.action_delay_max=3"])
    cm = _cm()
    flat = init_flat_params(3, cm.obs_size(True), cm.nu, EH)
    device = {} if be.name == "emu" else {"device": "cuda:0"}
    got = evaluate(cfg, flat, lib=be.lib, xp=be.xp, **device)
    assert got.episodes == r.episodes and np.array_equal(_bits(got.trajectory["qpos"]), _bits(traj[..., :cm.nq]))
    assert np.array_equal(_bits(got.trajectory["applied_action"]), _bits(tapp)) and np.array_equal(_bits(got.trajectory["action"]), _bits(traj[..., -cm.nu - 2:-2]))
    st = got.stats()
    assert st["obs_noise_level"] == 0.05 and st["obs_noise_qvel"] == 0.2 and st["action_delay_min"] == 0 and st["action_delay_max"] == 3 and "sensors" not in st
    # without the options the key set and the trajectory are what they were
    plain = evaluate(make_config(BASE, [f"model.hidden_size={EH}", f"evaluation.num_envs={EN}", "evaluation.num_steps=2", "evaluation.record_envs=1"]), flat, lib=be.lib,
                     xp=be.xp, **device)
    assert set(plain.stats()) == {"episodes", "mean_return", "std_return", "min_return", "max_return", "mean_length", "min_length", "max_length", "survivors",
                                  "survivor_mean_return", "mean_reward", "steps"} and set(plain.trajectory) == {"qpos", "qvel", "action", "reward", "done"}
    only_noise = evaluate(make_config(BASE, [f"model.hidden_size={EH}", f"evaluation.num_envs={EN}", "evaluation.num_steps=2", "evaluation.record_envs=1",
                                             "environment.obs_noise_level=1"]), flat, lib=be.lib, xp=be.xp, **device)
    assert "applied_action" not in only_noise.trajectory and "action_delay_max" not in only_noise.stats() and only_noise.stats()["obs_noise_level"] == 1.0
