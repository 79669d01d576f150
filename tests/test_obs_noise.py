"""Sensor noise: the noise stage (csrc/k_sensor.hip `mppo_obs_noise_apply`) against its host restatement (`jaxrng.obs_noise_philox`), "off is off" for both
sensor options in the engine, and the host surface (config keys, `HumanoidEnv`, the command line).  The engine's and the evaluator's compositions under noise
AND latency are in tests/test_action_delay.py.  Every comparison is bit for bit.

Sizes: the smallest built-in robot's long (O = 225, OP = 228) and short (O = 49) observation and the ball-joint humanoid's (O = 215, 71); N = 1, 5, 67 (67 rows of
57 blocks: fifteen workgroups of 256 lanes, the last one partly empty); the smallest engine tests/test_time_limit.py uses (8 environments, 4 steps)."""

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
from minppo_amd.train import obs_noise_scales

f32 = np.float32
ROOT = Path(__file__).resolve().parent.parent
BASE = {"kscale_id": "5eb3cb7f23232298", "visualization": {"camera_name": "track"}}
BALL = str(ROOT / "tests" / "golden" / "ball_joints" / "ball_humanoid.xml")
SEED = 5
NE, TE = 8, 4
ENGINE = [f"training.num_envs={NE}", f"training.num_steps={TE}", f"rl.num_env_steps={TE}", "training.num_minibatches=2", "training.update_epochs=2", "model.hidden_size=32",
          "training.total_timesteps=100000"]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _ncfg(rank=0, seed=SEED):
    return nat.ObsNoiseCfg(seed=seed, rank=rank, reserved=0)


def _sigma(O, rng):
    """A half-width per column with zeros in it: single zero columns, a whole Philox block of zeros, a block with one live column."""
    s = rng.uniform(0.01, 0.5, O).astype(f32)
    s[rng.random(O) < 0.2] = 0
    s[8:12] = 0
    s[16:20] = 0
    s[17] = 0.25
    s[0], s[O - 1] = 0.125, 0.0625  # (the first and the last column are noisy: the row's ends)
    return s


def _apply(be, obs, sigma, step_args, rank=0, seed=SEED, O=None, obs_ld=None, offset=0):
    """-> the observation after one mppo_obs_noise_apply; `offset` floats shift the base (an unaligned base takes the one-column form)."""
    N, ld = obs.shape
    O = sigma.size if O is None else O
    OP = (O + 3) & ~3
    buf = be.zeros((offset + N * ld,))
    be.put(buf, np.concatenate([np.zeros(offset, f32), obs.reshape(-1)]))
    table = np.zeros(OP, f32)
    table[:O] = sigma[:O]
    sig = be.arr(table)
    ctr, mul, add = step_args
    cdev = None if ctr is None else be.arr(np.array([ctr, 12345], np.int32))
    be.lib.obs_noise_apply(C.byref(_ncfg(rank, seed)), N, O, be.ptr(buf) + 4 * offset, ld if obs_ld is None else obs_ld, be.ptr(sig), be.ptr(cdev), mul, add, be.stream)
    be.sync()
    return be.host(buf)[offset:].reshape(N, ld).copy()


def _want(obs, sigma, step, rank=0, seed=SEED):
    N, O = obs.shape[0], sigma.size
    noise = jaxrng.obs_noise_philox(seed, rank, step, N, sigma)
    assert noise.shape == (N, O) and noise.dtype == f32 and (np.abs(noise) <= sigma).all() and (noise[:, sigma == 0] == 0).all()
    out = obs.copy()
    out[:, :O] = np.where(sigma > 0, obs[:, :O] + noise, obs[:, :O])
    return out, noise


OBS_SIZES = [225, 49, 215, 71]  # synth_stompy_pro with and without c-values, the ball-joint humanoid with and without


def test_observation_sizes_are_the_robots():
    pro, ball = load_model("synth_stompy_pro"), load_model(BALL)
    assert [pro.obs_size(True), pro.obs_size(False), ball.obs_size(True), ball.obs_size(False)] == OBS_SIZES and int(ball.t.get("nball", 0)) > 0


@pytest.mark.parametrize("O", OBS_SIZES)
@pytest.mark.parametrize("N", [1, 5, 67])
def test_noise_stage_equals_the_restatement(be, O, N):
    rng = np.random.default_rng(O * 100 + N)
    OP = (O + 3) & ~3
    sigma = _sigma(O, rng)
    zero_cols = np.flatnonzero(sigma == 0)
    assert zero_cols.size > 4 and (sigma > 0).sum() > O // 2
    for ld, offset in ((OP, 0), (OP + 3, 0), (OP, 1)):  # 16-byte rows; rows that are not; 16-byte rows from an unaligned base
        obs = rng.standard_normal((N, ld)).astype(f32)
        # sentinels where nothing may be written: -0.0 and a NaN with a payload in zero-sigma columns, NaNs in the pad columns and behind them
        obs[:, zero_cols[0]] = -0.0
        _bits(obs)[:, zero_cols[1]] = 0x7FC12345
        _bits(obs)[:, O:] = 0x7FC0BEEF
        for step, rank in ((0, 0), (1, 0), (2**32 - 1, 0), (1, 7)):
            got = _apply(be, obs, sigma, (None, 0, step if step < 2**31 else step - 2**32), rank=rank, offset=offset)
            want, noise = _want(obs, sigma, step, rank)
            assert np.array_equal(_bits(got), _bits(want)), (ld, offset, step, rank)
            assert np.array_equal(_bits(got[:, zero_cols]), _bits(obs[:, zero_cols])) and np.array_equal(_bits(got[:, O:]), _bits(obs[:, O:]))
            assert (_bits(got[:, zero_cols[0]]) == 0x80000000).all() and (_bits(got[:, zero_cols[1]]) == 0x7FC12345).all()
            assert (got[:, :O][:, sigma > 0] != obs[:, :O][:, sigma > 0]).mean() > 0.9
    # the draws differ between steps, ranks, seeds and environments, and fill the interval
    a, b, c, d = (_want(obs, sigma, s, r, sd)[1] for s, r, sd in ((1, 0, SEED), (2, 0, SEED), (1, 7, SEED), (1, 0, SEED + 1)))
    live = sigma > 0
    assert all((a[:, live] != x[:, live]).mean() > 0.99 for x in (b, c, d))
    if N > 1:
        assert (a[0, live] != a[1, live]).mean() > 0.99
    if N == 67:
        u = a[:, live] / sigma[live]
        # U(-1, 1) over k samples: the mean's deviation is 0.577 / sqrt(k), the standard deviation's sqrt((1/5 - 1/9) / k) / (2 * 0.577) = 0.258 / sqrt(k); four of each
        k = u.size
        assert k > 2000 and abs(u.mean()) < 4 * 0.577 / np.sqrt(k) and abs(u.std() - 1 / np.sqrt(3)) < 4 * 0.258 / np.sqrt(k) and u.min() < -0.99 and u.max() > 0.99


def test_noise_stage_reads_its_step_from_the_device_counter(be):
    O, N = 225, 5
    rng = np.random.default_rng(3)
    sigma, obs = _sigma(O, rng), rng.standard_normal((N, 228)).astype(f32)
    for ctr, mul, add in ((0, 4, 1), (3, 4, 2), (7, 0, 5), (2**31 - 1, 2, 1), (-1, 1, 0)):
        step = ((ctr & 0xFFFFFFFF) * mul + add) & 0xFFFFFFFF
        got = _apply(be, obs, sigma, (ctr, mul, add))
        assert np.array_equal(_bits(got), _bits(_want(obs, sigma, step)[0])), (ctr, mul, add)
        assert np.array_equal(_bits(got), _bits(_apply(be, obs, sigma, (None, 0, step if step < 2**31 else step - 2**32))))
    # a narrower O on the same rows: the columns behind it are pad
    got = _apply(be, obs, sigma, (None, 0, 1), O=49)
    assert np.array_equal(_bits(got[:, 49:]), _bits(obs[:, 49:])) and np.array_equal(_bits(got[:, :49]), _bits(_want(obs, sigma[:49], 1)[0][:, :49]))


def test_noise_stage_refusals(be):
    O, N = 49, 5
    obs, sig = be.zeros((N, 52)), be.zeros((52,))
    f = be.lib._fn["mppo_obs_noise_apply"]
    ok = lambda: f(C.byref(_ncfg()), N, O, be.ptr(obs), 52, be.ptr(sig), 0, 0, 0, be.stream)
    assert ok() == 0
    assert f(None, N, O, be.ptr(obs), 52, be.ptr(sig), 0, 0, 0, be.stream) == -1
    assert f(C.byref(_ncfg()), N, O, 0, 52, be.ptr(sig), 0, 0, 0, be.stream) == -1 and "null" in be.lib.last_error()
    assert f(C.byref(_ncfg()), N, O, be.ptr(obs), 52, 0, 0, 0, 0, be.stream) == -1
    assert f(C.byref(_ncfg(rank=256)), N, O, be.ptr(obs), 52, be.ptr(sig), 0, 0, 0, be.stream) == -1 and "256" in be.lib.last_error()
    assert f(C.byref(_ncfg(rank=-1)), N, O, be.ptr(obs), 52, be.ptr(sig), 0, 0, 0, be.stream) == -1
    assert f(C.byref(_ncfg()), N, O, be.ptr(obs), 51, be.ptr(sig), 0, 0, 0, be.stream) == -1 and "obs_ld 51" in be.lib.last_error()
    assert f(C.byref(_ncfg()), 0, O, be.ptr(obs), 52, be.ptr(sig), 0, 0, 0, be.stream) == -1
    assert f(C.byref(_ncfg()), N, 0, be.ptr(obs), 52, be.ptr(sig), 0, 0, 0, be.stream) == -1
    assert f(C.byref(_ncfg()), N, 4 * 65536 + 1, be.ptr(obs), 4 * 65536 + 4, be.ptr(sig), 0, 0, 0, be.stream) == -1 and "16 bits" in be.lib.last_error()
    be.sync()
    # a negative sigma: refused where the vector comes from the host - the engine's setter (and mppo_evaluate_sensors: tests/test_action_delay.py) - and by the restatement
    tr = be.trainer(make_config(BASE, ENGINE))
    g = be.lib._fn["mppo_engine_set_obs_noise"]
    bad = np.full(tr.O, 0.1, f32)
    bad[7] = -0.5
    assert g(tr._engine, bad.ctypes.data) == -1 and "column 7" in be.lib.last_error() and "negative" in be.lib.last_error()
    bad[7] = np.nan
    assert g(tr._engine, bad.ctypes.data) == -1
    assert g(None, bad.ctypes.data) == -1
    tr.close()
    with pytest.raises(ValueError):
        jaxrng.obs_noise_philox(1, 0, 0, 2, bad)
    with pytest.raises(ValueError):
        jaxrng.action_delays_philox(1, 0, 2, 3, 2)


# ---- off is off ---------------------------------------------------------------------------------------------------------------------------------------------------

_NAMES = ("params", "adam_m", "adam_v", "count", "state", "obs", "action", "reward", "done", "value", "adv", "target", "episode_returns", "episode_lengths", "timestep",
          "action_hist", "action_applied", "action_delay", "obs_noise_scale")


def _run(be, cfg, updates, before=None, **kw):
    tr = be.trainer(cfg, **kw)
    if before is not None:
        before(tr)
    tr.reset()
    for _ in range(updates):
        tr.update()
    tr._sync()
    out = {n: np.array(tr._to_host(tr.region(n))) for n in _NAMES}
    graph = tr.graph_active()
    tr.close()
    return out, graph


def test_options_off_is_an_engine_that_never_heard_of_them(be):
    cfg = make_config(BASE, ENGINE)
    never, g_never = _run(be, cfg, 2)

    def setters(tr):
        be.lib.engine_set_obs_noise(tr._engine, np.zeros(tr.O, f32).ctypes.data)
        be.lib.engine_set_obs_noise(tr._engine, None)
        be.lib.engine_set_action_delay(tr._engine, 0, 0)

    zero, g_zero = _run(be, cfg, 2, before=setters)
    keyed, g_keyed = _run(be, make_config(BASE, ENGINE + ["environment.obs_noise_level=0", "environment.obs_noise_qvel=3", "environment.action_delay_min=0",
                                                          "environment.action_delay_max=0"]), 2)
    assert g_never == g_zero == g_keyed == (be.name == "hip")
    for k in never:
        assert np.array_equal(never[k].view(np.uint8), zero[k].view(np.uint8)) and np.array_equal(never[k].view(np.uint8), keyed[k].view(np.uint8)), k
    # the four regions are there, and untouched
    assert never["action_hist"].size == 16 * NE * 10 and never["action_applied"].size == NE * 10 and never["action_delay"].size == NE and never["obs_noise_scale"].size == 228
    assert not any(never[k].view(np.uint8).any() for k in ("action_hist", "action_applied", "action_delay", "obs_noise_scale"))
    # ... and either option changes the run
    noisy, _ = _run(be, make_config(BASE, ENGINE + ["environment.obs_noise_level=1"]), 2)
    late, _ = _run(be, make_config(BASE, ENGINE + ["environment.action_delay_min=1", "environment.action_delay_max=2"]), 2)
    assert not np.array_equal(noisy["obs"], never["obs"]) and not np.array_equal(late["state"], never["state"])
    assert np.array_equal(noisy["obs_noise_scale"][:225], obs_noise_scales(make_config(BASE, ["environment.obs_noise_level=1"]), load_model("synth_stompy_pro")))
    assert np.array_equal(late["action_delay"], jaxrng.action_delays_philox(1337, 0, NE, 1, 2)) and late["action_hist"].any()


def test_setters_call_order_and_refusals(be):
    tr = be.trainer(make_config(BASE, ENGINE))
    f, g = be.lib._fn["mppo_engine_set_action_delay"], be.lib._fn["mppo_engine_set_obs_noise"]
    assert f(tr._engine, -1, 2) == -1 and "-1" in be.lib.last_error()
    assert f(tr._engine, 3, 2) == -1 and "3" in be.lib.last_error()
    assert f(tr._engine, 0, 17) == -1 and "17" in be.lib.last_error()
    assert f(None, 0, 1) == -1
    be.lib.engine_set_action_delay(tr._engine, 1, 16)
    be.lib.engine_set_action_delay(tr._engine, 0, 0)
    sig = np.full(tr.O, 0.1, f32)
    be.lib.engine_set_obs_noise(tr._engine, sig.ctypes.data)
    tr.reset()
    assert f(tr._engine, 0, 1) == -4 and "mppo_engine_reset has run" in be.lib.last_error()  # MPPO_ESTATE
    assert g(tr._engine, sig.ctypes.data) == -4 and "mppo_engine_reset has run" in be.lib.last_error()
    tr.lib.engine_prepare(tr._engine, tr._stream_ptr)
    tr._sync()
    assert f(tr._engine, 0, 1) == -4 and "prepared" in be.lib.last_error()
    assert g(tr._engine, None) == -4 and "prepared" in be.lib.last_error()
    tr.close()
    # any number of ranks: the rank enters the streams, nothing crosses ranks
    two = be.trainer(make_config(BASE, ENGINE + ["environment.obs_noise_level=1", "environment.action_delay_max=2"]), world_size=2, rank=1)
    assert two.obs_noise is not None and two.action_delay.max == 2 and two.action_delay.rank == 1
    two.close()


# ---- the host surface ---------------------------------------------------------------------------------------------------------------------------------------------


def test_config_keys_defaults_and_refusals():
    env = make_config(BASE).environment
    assert (env.obs_noise_level, env.obs_noise_qpos, env.obs_noise_qvel, env.obs_noise_cinert, env.obs_noise_cvel, env.obs_noise_qfrc) == (0.0, 0.01, 0.2, 0.0, 0.1, 0.0)
    assert (env.action_delay_min, env.action_delay_max) == (0, 0)
    for bad in ("obs_noise_level=-1", "obs_noise_qpos=-0.1", "obs_noise_qvel=-1", "obs_noise_cinert=-1", "obs_noise_cvel=-1", "obs_noise_qfrc=-2", "obs_noise_level=.nan"):
        with pytest.raises(ValueError, match="sensor noise"):
            make_config(BASE, ["environment." + bad])
    for bad in (["action_delay_min=-1"], ["action_delay_min=2", "action_delay_max=1"], ["action_delay_max=17"], ["action_delay_min=1"]):
        with pytest.raises(ValueError, match="latency"):
            make_config(BASE, ["environment." + b for b in bad])
    ok = make_config(BASE, ["environment.action_delay_min=16", "environment.action_delay_max=16", "environment.obs_noise_level=2.5"])
    assert ok.environment.action_delay_max == 16
    # the per-column vector follows the observation's layout, with and without c-values, on both robots
    for name in ("synth_stompy_pro", BALL):
        cm = load_model(name)
        nb = cm.nbody - 1
        long = obs_noise_scales(make_config(BASE, ["environment.obs_noise_level=2", "environment.obs_noise_cinert=0.5", "environment.obs_noise_qfrc=0.25"]), cm)
        want = np.concatenate([np.full(cm.nq, 0.02), np.full(cm.nv, 0.4), np.full(10 * nb, 1.0), np.full(6 * nb, 0.2), np.full(cm.nv, 0.5)]).astype(f32)
        assert long.dtype == f32 and np.array_equal(long, want) and long.size == cm.obs_size(True)
        short = obs_noise_scales(make_config(BASE, ["environment.obs_noise_level=1", "environment.include_c_vals=false"]), cm)
        assert np.array_equal(short, np.concatenate([np.full(cm.nq, 0.01), np.full(cm.nv, 0.2), np.zeros(cm.nv)]).astype(f32)) and short.size == cm.obs_size(False)
        assert obs_noise_scales(make_config(BASE), cm) is None
        assert obs_noise_scales(make_config(BASE, ["environment.obs_noise_level=1", "environment.obs_noise_qpos=0", "environment.obs_noise_qvel=0", "environment.obs_noise_cvel=0"]), cm) is None


def test_two_ranks_draw_from_streams_of_their_own(be):
    """Pure draws: no second process.  Each rank's latency table and noise equal their restatements, and the two ranks' differ."""
    N, O = 67, 49
    tables = []
    for rank in (0, 1):
        d = be.full((N,), -7, np.int32)
        be.lib.action_delay_fill(C.byref(nat.ActionDelayCfg(min=0, max=16, rank=rank, reserved=0, seed=SEED)), N, be.ptr(d), be.stream)
        be.sync()
        tables.append(be.host(d).copy())
        assert np.array_equal(tables[-1], jaxrng.action_delays_philox(SEED, rank, N, 0, 16))
    assert (tables[0] != tables[1]).mean() > 0.8
    rng = np.random.default_rng(0)
    sigma, obs = _sigma(O, rng), rng.standard_normal((N, 52)).astype(f32)
    r0, r1 = (_apply(be, obs, sigma, (None, 0, 3), rank=r) for r in (0, 1))
    assert np.array_equal(_bits(r0), _bits(_want(obs, sigma, 3, 0)[0])) and np.array_equal(_bits(r1), _bits(_want(obs, sigma, 3, 1)[0]))
    assert (r0[:, :O][:, sigma > 0] != r1[:, :O][:, sigma > 0]).mean() > 0.99


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ["synth_stompy_pro", BALL], ids=["stompy_pro", "ball_humanoid"])
def test_humanoid_env_applies_noise_and_latency(robot):
    """reset / step with both options against the stage entry points' restatements: the observation is the plain environment's plus
    `obs_noise_philox`, and the step is the plain environment's step under the delayed action."""
    import torch

    from minppo_amd.env import HumanoidEnv

    N, D, K = 5, 3, 6
    opts = [f"environment.model={robot}", "environment.obs_noise_level=1", "environment.obs_noise_cinert=0.05", "environment.action_delay_min=0",
            f"environment.action_delay_max={D}", "environment.episode_length=4", f"training.seed={SEED}"]
    env, plain = HumanoidEnv(make_config(BASE, opts)), HumanoidEnv(make_config(BASE, [f"environment.model={robot}", "environment.episode_length=4"]))
    O, A = env.observation_size, env.action_size
    sigma = env.obs_noise_scales()
    assert sigma.shape == (O,) and (sigma > 0).sum() > O // 2
    delays = env.action_delays(N).cpu().numpy()
    assert np.array_equal(delays, jaxrng.action_delays_philox(SEED, 0, N, 0, D)) and delays.min() == 0 and delays.max() > 0
    assert np.array_equal(env.action_delays(N, seed=9).cpu().numpy(), jaxrng.action_delays_philox(9, 0, N, 0, D))
    es, ps = env.reset(num_envs=N), plain.reset(num_envs=N)
    assert es.action_history.shape == (D, N, A) and not es.action_history.any() and ps.action_history is None and len(ps) == 6
    noisy = lambda plain_state, step: (plain_state.obs.cpu().numpy() + jaxrng.obs_noise_philox(SEED, 0, step, N, sigma)).astype(f32)  # (the plain environment's observation is the exact one)
    live = sigma > 0
    assert np.array_equal(_bits(es.obs.cpu().numpy()[:, live]), _bits(noisy(ps, 0)[:, live])) and torch.equal(es.pipeline_state, ps.pipeline_state)
    assert np.array_equal(_bits(es.obs.cpu().numpy()[:, ~live]), _bits(ps.obs.cpu().numpy()[:, ~live]))
    gen = np.random.default_rng(1)
    acts = (0.3 * gen.standard_normal((K, N, A))).astype(f32)
    for k in range(K):
        ep = es.metrics.episode_lengths.cpu().numpy()
        want = np.zeros((N, A), f32)
        for n in range(N):
            if delays[n] == 0:
                want[n] = acts[k, n]
            elif ep[n] >= delays[n]:
                want[n] = acts[k - delays[n], n]
        es = env.step(es, torch.from_numpy(acts[k]).to(env.device))
        ps = plain.step(ps, torch.from_numpy(want).to(env.device))
        assert torch.equal(es.pipeline_state, ps.pipeline_state) and torch.equal(es.reward, ps.reward) and torch.equal(es.done, ps.done), k
        assert int(es.metrics.timestep[0]) == k + 1
        assert np.array_equal(_bits(es.obs.cpu().numpy()[:, live]), _bits(noisy(ps, k + 1)[:, live])), k
        assert np.array_equal(_bits(es.obs.cpu().numpy()[:, ~live]), _bits(ps.obs.cpu().numpy()[:, ~live]))
        assert torch.equal(es.action_history[k % D], torch.from_numpy(acts[k]).to(env.device))
    assert bool(es.truncation is not None) and int(es.metrics.returned_episode_lengths[0]) == 4  # (a restart lay inside the run: zeros after it)
    env.close()
    plain.close()


@pytest.mark.gpu
def test_evaluate_echoes_the_keys_from_the_command_line(tmp_path):
    model = str(tmp_path / "model.pkl")
    small = ["training.num_envs=64", "training.num_minibatches=2", "model.hidden_size=64", "environment.obs_noise_level=1", "environment.action_delay_min=1",
             "environment.action_delay_max=2"]
    p = subprocess.run([sys.executable, "-m", "minppo_amd.cli", "train", "stompy_pro", *small, "training.total_timesteps=1280", f"training.model_save_path={model}"],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert p.returncode == 0 and Path(model).exists(), p.stderr[-2000:]
    traj = str(tmp_path / "traj.npz")
    p = subprocess.run([sys.executable, "-m", "minppo_amd.cli", "evaluate", "stompy_pro", *small, "evaluation.num_envs=20", "evaluation.num_steps=8", "evaluation.record_envs=3",
                        f"evaluation.trajectory_path={traj}", f"inference.model_path={model}"], capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1
    out = json.loads(line[0])
    assert out["steps"] == 160 and out["obs_noise_level"] == 1.0 and out["obs_noise_qvel"] == 0.2 and out["action_delay_min"] == 1 and out["action_delay_max"] == 2
    assert {"obs_noise_qpos", "obs_noise_cinert", "obs_noise_cvel", "obs_noise_qfrc"} <= set(out)
    with np.load(traj) as z:
        d = jaxrng.action_delays_philox(1337, 0, 3, 1, 2)
        act, app = z["action"], z["applied_action"]
        assert app.shape == act.shape == (9, 3, 10) and not app[0].any()
        for n in range(3):  # nobody falls in eight steps: one episode, the policy's action d steps late behind d zero steps
            assert not app[1:1 + d[n], n].any() and np.array_equal(_bits(app[1 + d[n]:, n]), _bits(act[1:9 - d[n], n]))
