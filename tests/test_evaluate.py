"""Policy evaluation (`mppo_evaluate`, csrc/evaluator.hip / k_eval.hip; `minppo_amd.evaluate`, `Trainer.evaluate`, `cli evaluate`).

A. `mppo_evaluate` IS the composition of the library's own entry points: the test drives mppo_env_reset, [mppo_env_reinit], then K rounds of
   mppo_normal_fill (or zeros), mppo_policy_forward, mppo_env_step, [mppo_env_reinit over done] through the ABI on the same backend, snapshots
   state / action / reward / done / metrics every step, and asks of mppo_evaluate on the same inputs: the trajectory bit for bit, counts and
   min / max equal to NumPy's on the snapshots, the four double sums within 1e-12 * sum|x| of NumPy's float64 (at most N + K additions, each
   rounding by 2^-53: <= 1.3e-13 at the largest N used in these tests).
C. a short check of the same numbers against the float64 oracle, at the tolerances tests/test_env_surface.py holds the same kernels to.
D. refusals.    E. the Python layer and the command line.
(B, the statistics stages alone, is tests/test_eval_stats.py.)

Shapes: robot synth_stompy_pro, N = 20 environments (five waves of four, one workgroup and a part), H = 64, R = 7 recorded environments (a strict,
odd subset).  What each case has to contain is asserted of the COMPOSED run, so a drift of the inputs cannot hollow a case out: at least one ended
episode and at least one survivor - except case "masked", whose window ends episodes at every step in every environment (there: more ended
episodes than environments, i.e. the accumulators see several episodes of one environment, and a masked reinit at every step)."""

import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from minppo_amd import _native as nat
from minppo_amd import jaxrng
from minppo_amd.config import MissingMandatoryValue, make_config
from minppo_amd.model import load_model
from minppo_amd.train import flat_to_tree, init_flat_params, reward_cfg
from physics_harness import GOLDEN, METRIC_TYPES

f32 = np.float32
ROOT = Path(__file__).resolve().parent.parent
BASE = {"kscale_id": "5eb3cb7f23232298", "visualization": {"camera_name": "track"}}
N, H, R = 20, 64, 7

#        K  n_frames  deterministic  reset noise  height window   include_c_vals  bf16  robot
CASES = {
    "stochastic": dict(K=16, n_frames=5, det=0, noise=0.0, window=(-0.2, 1.015)),
    "deterministic_noise": dict(K=12, n_frames=1, det=1, noise=0.01, window=(1.005, 2.0)),
    "masked": dict(K=16, n_frames=5, det=0, noise=0.01, window=(1.005, 1.012)),
    "short_obs": dict(K=16, n_frames=5, det=0, noise=0.0, window=(-0.2, 1.015), c_vals=False),
    "bf16": dict(K=16, n_frames=5, det=0, noise=0.0, window=(-0.2, 1.015), bf16=1),
    "export_biped": dict(K=3, n_frames=5, det=0, noise=0.01, window=(0.918, 2.0), robot=str(GOLDEN / "export_biped" / "robot.xml")),
}
SEED = 5
_CM, _COMPOSED, _EVAL = {}, {}, {}


def _case(name):
    c = dict(c_vals=True, bf16=0, robot="synth_stompy_pro")
    c.update(CASES[name])
    return c


def _cm(robot):
    if robot not in _CM:
        _CM[robot] = load_model(robot)
    return _CM[robot]


def _rc(window):
    return reward_cfg(make_config(BASE, [f"reward.height_min_z={window[0]}", f"reward.height_max_z={window[1]}"]))


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _open(be, c):
    cm = _cm(c["robot"])
    h, dims, keep = be.model(cm, c["c_vals"])
    net = nat.Net(dims.obs_dim, dims.obs_pad, dims.nu, H, 1, c["bf16"], 2)
    params = init_flat_params(3, dims.obs_dim, dims.nu, H)
    return cm, h, dims, keep, net, params


def _ecfg(c, n=N, k=None, r=R):
    return nat.EvalCfg(N=n, K=c["K"] if k is None else k, n_frames=c["n_frames"], deterministic=c["det"], record_envs=r, reset_noise_scale=c["noise"], seed=SEED,
                       reward=_rc(c["window"]))


def composed(be, name):
    """The evaluation written out with the library's own entry points -> the snapshots of every step (computed once per backend and case)."""
    key = (be.name, name)
    if key in _COMPOSED:
        return _COMPOSED[key]
    c = _case(name)
    cm, h, dims, keep, net, params = _open(be, c)
    K, OP, RD, A, nqv = c["K"], dims.obs_pad, dims.rec_dim, dims.nu, cm.nq + cm.nv
    lib, s = be.lib, be.stream
    state, rec, obs = be.zeros((N, RD)), be.zeros((RD,)), be.zeros((N, OP))
    rew, done = be.zeros((N,)), be.zeros((N,), np.uint8)
    met = {k: be.full((N,), 3, t) for k, t in METRIC_TYPES.items()}  # (the reset zeroes them)
    M = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    p_dev = be.arr(params)
    act, logp, val, noise = be.zeros((N, A)), be.zeros((N,)), be.zeros((N,)), be.zeros((N, A))
    wsb = lib.policy_ws_bytes(C.byref(net), N)
    ws = be.zeros((wsb,), np.uint8)
    rc = _rc(c["window"])
    lib.env_reset(h, N, be.ptr(state), be.ptr(rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(M), s)
    if c["noise"] > 0:
        lib.env_reinit(h, N, be.ptr(state), be.ptr(obs), OP, 0, c["noise"], 0, SEED, 0, 0, 0, 0, s)
    out = dict(state=[be.host(state)[:, :nqv].copy()], obs0=be.host(obs).copy(), action=[], reward=[], done=[], met=[])
    for t in range(K):
        if not c["det"]:
            lib.normal_fill(SEED, t, N * A, be.ptr(noise), s)
        lib.policy_forward(C.byref(net), be.ptr(p_dev), N, be.ptr(obs), OP, be.ptr(noise), be.ptr(act), be.ptr(logp), be.ptr(val), 0, be.ptr(ws), wsb, s)
        lib.env_step(h, N, c["n_frames"], C.byref(rc), be.ptr(state), be.ptr(rec), be.ptr(act), A, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(M), s)
        if c["noise"] > 0:
            lib.env_reinit(h, N, be.ptr(state), be.ptr(obs), OP, be.ptr(done), c["noise"], 0, SEED, 0, 0, 0, t + 1, s)
        be.sync()
        out["state"].append(be.host(state)[:, :nqv].copy())
        out["action"].append(be.host(act).copy()); out["reward"].append(be.host(rew).copy()); out["done"].append(be.host(done).copy())
        out["met"].append({k: be.host(v).copy() for k, v in met.items()})
    lib.model_close(h)
    out = {k: (np.stack(v) if k in ("state", "action", "reward", "done") else v) for k, v in out.items()}
    out.update(nq=cm.nq, nv=cm.nv, A=A, cm=cm)
    _COMPOSED[key] = out
    return out


def evaluated(be, name, fill=0xA5):
    """mppo_evaluate on the inputs of `composed` -> (result struct, its bytes, trajectory [K + 1, R, W]).  The workspace starts as garbage."""
    key = (be.name, name, fill)
    if key in _EVAL:
        return _EVAL[key]
    c = _case(name)
    cm, h, dims, keep, net, params = _open(be, c)
    e = _ecfg(c)
    need = be.lib.eval_ws_bytes(h, C.byref(net), C.byref(e))
    assert need > 0
    ws = be.full((need,), fill, np.uint8)
    res = be.full((C.sizeof(nat.EvalResultRaw) // 8,), -1, np.int64)
    W = cm.nq + cm.nv + dims.nu + 2
    traj = be.full((c["K"] + 1, R, W), np.nan)
    p_dev = be.arr(params)
    be.lib.evaluate(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), need, be.ptr(res), be.ptr(traj), be.stream)
    be.sync()
    raw = be.host(res).tobytes()
    out = (nat.EvalResultRaw.from_buffer_copy(raw), raw, be.host(traj).copy())
    be.lib.model_close(h)
    _EVAL[key] = out
    return out


def numpy_stats(snap):
    """What the result struct must hold, from the snapshots, in NumPy float64 / int64."""
    fin = np.stack([m["returned_episode"] for m in snap["met"]]) != 0
    rets = np.stack([m["returned_episode_returns"] for m in snap["met"]])[fin].astype(np.float64)
    lens = np.stack([m["returned_episode_lengths"] for m in snap["met"]])[fin].astype(np.int64)
    surv = ~fin.any(0)
    run = snap["met"][-1]["episode_returns"].astype(np.float64)[surv]
    rew = snap["reward"].astype(np.float64)
    return dict(fin=fin, episodes=int(fin.sum()), len_sum=int(lens.sum()), len_min=int(lens.min()) if lens.size else 0, len_max=int(lens.max()) if lens.size else 0,
                survivors=int(surv.sum()), steps=fin.size, ret_min=rets.min() if rets.size else np.inf, ret_max=rets.max() if rets.size else -np.inf,
                sums=dict(ret_sum=rets, ret_sumsq=rets * rets, survivor_ret_sum=run, reward_sum=rew.reshape(-1)))


def check_result(r, want):
    for k in ("episodes", "len_sum", "len_min", "len_max", "survivors", "steps"):
        assert getattr(r, k) == want[k], (k, getattr(r, k), want[k])
    assert r.ret_min == want["ret_min"] and r.ret_max == want["ret_max"]
    for k, x in want["sums"].items():
        got, ref, scale = getattr(r, k), float(x.sum()), float(np.abs(x).sum())
        print(f"{k}: got {got!r} numpy {ref!r} |diff| {abs(got - ref):.3e} bound {1e-12 * scale:.3e}")
        assert abs(got - ref) <= 1e-12 * scale, (k, got, ref)


def check_case(be, name):
    snap, (r, raw, traj) = composed(be, name), evaluated(be, name)
    want = numpy_stats(snap)
    fin = want["fin"]
    print(f"{name}: {want['episodes']} episodes ended (per step {fin.sum(1).tolist()}, per environment {fin.sum(0).tolist()}), {want['survivors']} survivors")
    assert np.array_equal(fin, snap["done"] != 0)
    assert want["episodes"] >= 1
    if name == "masked":
        assert want["episodes"] > N and fin.any(1).all()  # several episodes per environment, a masked reinit with work at every step
    else:
        assert want["survivors"] >= 1
    nqv, A = snap["nq"] + snap["nv"], snap["A"]
    assert not np.isnan(traj).any()
    assert np.array_equal(_bits(traj[:, :, :nqv]), _bits(snap["state"][:, :R])), "state rows"
    assert (traj[0, :, nqv:] == 0).all(), "frame 0: zero action / reward / done"
    assert np.array_equal(_bits(traj[1:, :, nqv:nqv + A]), _bits(snap["action"][:, :R])), "action"
    assert np.array_equal(_bits(traj[1:, :, nqv + A]), _bits(snap["reward"][:, :R])), "reward"
    assert np.array_equal(traj[1:, :, nqv + A + 1], (snap["done"][:, :R] != 0).astype(f32)), "done"
    check_result(r, want)
    # the same inputs, another garbage in the workspace: the same bytes
    assert evaluated(be, name, fill=0x3C)[1] == raw


# ---- A: bit-equality with the composition of existing entry points -------------------------------------------------------------------------


@pytest.mark.parametrize("name", [n for n in CASES if n != "export_biped"])
def test_evaluate_is_the_composition_of_the_entry_points(be, name):
    check_case(be, name)


@pytest.mark.gpu
def test_evaluate_is_the_composition_on_a_robot_with_matrices_in_global_memory():
    """The export biped (33 dofs, 19 contact slots: mass matrix and Jacobian in global memory, here a region of the evaluator's workspace, in the
    composed run the handle's own allocation), on its specialised kernel: on the device.  Window: the pelvis stands at 0.91 - 0.93 after the noisy
    reset, so a floor of 0.918 ends about a third of the episodes at the first step and leaves the rest standing."""
    from backends import get_backend

    be = get_backend("hip")
    c = _case("export_biped")
    cm, h, dims, keep, net, params = _open(be, c)
    sb = C.c_size_t(0)
    be.lib.model_scratch_bytes(h, N, C.byref(sb))
    be.lib.model_close(h)
    assert sb.value > 0
    check_case(be, "export_biped")


def test_deterministic_actions_are_the_means(be):
    """With the zero noise buffer the action column is `mean_out` of mppo_policy_forward on the same observation, bit for bit (frame 1: the
    observation after the reset and the initial reinit)."""
    c = _case("deterministic_noise")
    snap, (_, _, traj) = composed(be, "deterministic_noise"), evaluated(be, "deterministic_noise")
    cm, h, dims, keep, net, params = _open(be, c)
    A, OP = dims.nu, dims.obs_pad
    obs, p_dev = be.arr(snap["obs0"]), be.arr(params)
    noise = be.arr((0.5 + np.arange(N * A, dtype=f32)).reshape(N, A))
    act, logp, val, mean = be.zeros((N, A)), be.zeros((N,)), be.zeros((N,)), be.zeros((N, (A + 3) & ~3))  # (mean_out rows are padded to four floats)
    wsb = be.lib.policy_ws_bytes(C.byref(net), N)
    ws = be.zeros((wsb,), np.uint8)
    be.lib.policy_forward(C.byref(net), be.ptr(p_dev), N, be.ptr(obs), OP, be.ptr(noise), be.ptr(act), be.ptr(logp), be.ptr(val), be.ptr(mean), be.ptr(ws), wsb, be.stream)
    be.sync()
    be.lib.model_close(h)
    nqv = cm.nq + cm.nv
    assert np.array_equal(_bits(traj[1, :, nqv:nqv + A]), _bits(be.host(mean)[:R, :A]))
    assert not np.array_equal(be.host(act), be.host(mean)[:, :A])


# ---- C: against the float64 oracle -----------------------------------------------------------------------------------------------------------


def test_first_steps_follow_the_float64_oracle(be):
    """Case "deterministic_noise", steps 0 .. 2, against oracle.env_oracle.EnvOracle driven by ppo_oracle.actor_critic_forward means from the host
    restatement of the reset noise (jaxrng.reset_noise_philox; an ended episode restarts from event t + 1's draw): `done` equal, the reset
    observation within atol 1e-5 and the rewards within atol 0.3 - the tolerances of tests/test_env_surface.py:41,48 for the same kernels."""
    from oracle import ppo_oracle as po
    from oracle.env_oracle import EnvOracle, RewardCfg

    c = _case("deterministic_noise")
    snap, (_, _, traj) = composed(be, "deterministic_noise"), evaluated(be, "deterministic_noise")
    cm, nq, nv, A = snap["cm"], snap["nq"], snap["nv"], snap["A"]
    orc = EnvOracle(cm.t, RewardCfg(height_min_z=c["window"][0], height_max_z=c["window"][1]), n_frames=c["n_frames"])
    q0 = np.asarray(cm.t["qpos0"], f32)

    def noisy(event):
        dq, dv = jaxrng.reset_noise_philox(SEED, 0, event, N, nq, nv, c["noise"])
        return orc.ph.pipeline_init((q0[None] + dq).astype(f32).astype(np.float64), dv.astype(np.float64))

    es = orc.reset(N)
    es["pipeline_state"] = noisy(0)
    es["obs"] = orc.get_obs(es["pipeline_state"])
    O = es["obs"].shape[1]
    np.testing.assert_allclose(snap["obs0"][:, :O], es["obs"], atol=1e-5)
    np.testing.assert_allclose(traj[0, :, :nq + nv], es["obs"][:R, :nq + nv], atol=1e-5)
    named = po.flat_to_named(init_flat_params(3, O, A, H).astype(np.float64), O, A, H)
    for t in range(3):
        mean, _, _ = po.actor_critic_forward(named, es["obs"], True)
        es = orc.step(es, mean)
        d = es["done"]
        assert np.array_equal(d[:R], traj[t + 1, :, nq + nv + A + 1] != 0) and np.array_equal(d, snap["done"][t] != 0), t
        np.testing.assert_allclose(traj[t + 1, :, nq + nv + A], es["reward"][:R], atol=0.3)
        np.testing.assert_allclose(snap["reward"][t], es["reward"], atol=0.3)
        if d.any():  # the reference's randomised restart (env.py:115-121, 179-180) where the oracle's step put the constant record
            fresh, s = noisy(t + 1), es["pipeline_state"]
            for k, v in s.items():
                if isinstance(v, np.ndarray) and v.shape[:1] == (N,) and k in fresh:
                    s[k] = np.where(d.reshape((N,) + (1,) * (v.ndim - 1)), fresh[k], v)
            es["obs"] = np.where(d[:, None], orc.get_obs(fresh), es["obs"])


# ---- D: refusals -----------------------------------------------------------------------------------------------------------------------------


def test_evaluate_refuses_bad_arguments(be):
    c = _case("stochastic")
    cm, h, dims, keep, net, params = _open(be, c)
    good = _ecfg(c, k=2)
    need = be.lib.eval_ws_bytes(h, C.byref(net), C.byref(good))
    ws, res = be.zeros((need,), np.uint8), be.zeros((12,), np.int64)
    traj = be.zeros((3, R, cm.nq + cm.nv + dims.nu + 2))
    p_dev = be.arr(params)

    def call(e, p=p_dev, w=ws, wb=need, r=res, tr=traj, model=h, n=net):
        be.lib.evaluate(model, C.byref(n) if n is not None else None, be.ptr(p), C.byref(e) if e is not None else None, be.ptr(w), wb, be.ptr(r), be.ptr(tr), be.stream)
        be.sync()

    for kw, msg in ((dict(e=_ecfg(c, n=0, k=2, r=0)), "N = 0"), (dict(e=_ecfg(c, k=0)), "K = 0"), (dict(e=_ecfg(c, k=2, r=N + 1)), "record_envs"),
                    (dict(e=good, p=None), "null"), (dict(e=good, w=None), "null"), (dict(e=good, r=None), "null"), (dict(e=good, tr=None), "null trajectory"),
                    (dict(e=None), "null"), (dict(e=good, n=None), "null"), (dict(e=good, model=None), "null"), (dict(e=good, wb=need - 1), "workspace")):
        with pytest.raises(nat.NativeError, match=msg):
            call(**kw)
    assert be.lib.eval_ws_bytes(h, C.byref(net), C.byref(_ecfg(c, k=0))) == 0
    call(good)  # the model is as it was: a valid call still works
    r = nat.EvalResultRaw.from_buffer_copy(be.host(res).tobytes())
    assert r.steps == 2 * N
    call(_ecfg(c, k=2, r=0), tr=None)  # no recorded environment: the trajectory may be null
    be.lib.model_close(h)


# ---- E: Python and command line ------------------------------------------------------------------------------------------------------------------

EVAL_OVERRIDES = ["model.hidden_size=64", f"training.seed={SEED}", f"evaluation.num_envs={N}", "evaluation.num_steps=16", f"evaluation.record_envs={R}",
                  "evaluation.deterministic=false", "environment.n_frames=5", "reward.height_min_z=-0.2", "reward.height_max_z=1.015"]


def test_python_evaluate_equals_the_abi_result(be, tmp_path):
    """Case "stochastic" through `minppo_amd.evaluate.evaluate`: a tree, a flat vector and a pickle path give the ABI's numbers."""
    from minppo_amd.evaluate import evaluate, result_from_struct
    from minppo_amd.train import save_model

    r, _, traj = evaluated(be, "stochastic")
    cfg = make_config(BASE, EVAL_OVERRIDES)
    cm = _cm("synth_stompy_pro")
    A = composed(be, "stochastic")["A"]
    O = cm.nq + 2 * cm.nv + 16 * (cm.nbody - 1)  # the full observation (env.py:245-253)
    flat = init_flat_params(3, O, A, H)
    tree = flat_to_tree(flat, O, A, H)
    path = str(tmp_path / "model.pkl")
    save_model(tree, path)
    want = result_from_struct(r)
    device = {} if be.name == "emu" else {"device": "cuda:0"}
    got = evaluate(cfg, tree, lib=be.lib, xp=be.xp, **device)
    assert got.stats() == want.stats()
    assert got.episodes >= 1 and got.survivors >= 1 and np.isfinite(list(got.stats().values())).all()
    nqv = cm.nq + cm.nv
    for k, cols in (("qpos", slice(0, cm.nq)), ("qvel", slice(cm.nq, nqv)), ("action", slice(nqv, nqv + A)), ("reward", nqv + A)):
        assert np.array_equal(_bits(got.trajectory[k]), _bits(traj[..., cols])), k
    assert got.trajectory["done"].dtype == bool and np.array_equal(got.trajectory["done"], traj[..., nqv + A + 1] != 0)
    # a tree, a flat vector and a pickle path are the same parameters (two steps: the emulator is slow)
    short = [evaluate(cfg, p, lib=be.lib, xp=be.xp, num_steps=2, **device) for p in (tree, flat, path, Path(path))]
    for o in short[1:]:
        assert o.stats() == short[0].stats() and all(np.array_equal(_bits(o.trajectory[k]), _bits(short[0].trajectory[k])) for k in o.trajectory)
    assert np.array_equal(_bits(short[0].trajectory["qpos"]), _bits(traj[:3, :, :cm.nq]))
    assert evaluate(cfg, flat, lib=be.lib, xp=be.xp, record_envs=0, num_steps=2, **device).trajectory is None
    with pytest.raises(ValueError, match="parameters"):
        evaluate(cfg, flat[:-4], lib=be.lib, xp=be.xp, **device)
    with pytest.raises(TypeError, match="bogus"):
        evaluate(cfg, flat, lib=be.lib, xp=be.xp, bogus=1, **device)


def test_no_finished_episode_gives_nan_not_a_division_by_zero(be):
    from minppo_amd.evaluate import evaluate

    cfg = make_config(BASE, ["model.hidden_size=64", "evaluation.num_envs=5", "evaluation.num_steps=2"])  # (the default window: nobody falls in two steps)
    flat = init_flat_params(3, 225, 10, H)
    got = evaluate(cfg, flat, lib=be.lib, xp=be.xp)
    assert got.episodes == 0 and got.survivors == 5 and got.steps == 10 and got.trajectory is None
    for k in ("mean_return", "std_return", "min_return", "max_return", "mean_length", "min_length", "max_length"):
        assert np.isnan(getattr(got, k)), k
    assert np.isfinite(got.survivor_mean_return) and np.isfinite(got.mean_reward)


def test_config_section_and_missing_model_path():
    from minppo_amd.evaluate import main

    ev = make_config(BASE).evaluation
    assert (ev.num_envs, ev.num_steps, ev.deterministic, ev.record_envs, ev.trajectory_path) == (256, 1000, True, 0, "")
    assert make_config(BASE, ["evaluation.num_envs=8", "evaluation.deterministic=false"]).evaluation.deterministic is False
    with pytest.raises(MissingMandatoryValue, match="inference.model_path"):
        main(["stompy_pro"])
    with pytest.raises(ValueError, match="record_envs"):  # refused before anything runs (the model file does not exist)
        main(["stompy_pro", "inference.model_path=/nonexistent/model.pkl", "evaluation.trajectory_path=t.npz"])


def test_cli_knows_evaluate(monkeypatch):
    from minppo_amd import cli

    monkeypatch.setattr(sys, "argv", ["minppo", "evaluate", "stompy_pro"])
    with pytest.raises(MissingMandatoryValue, match="inference.model_path"):
        cli.main()


@pytest.mark.gpu
def test_train_save_and_evaluate_from_the_command_line(tmp_path):
    """One update, save_model, `cli evaluate` twice (identical output, an .npz of [9, 3, .] arrays), and Trainer.evaluate() on the same trainer agrees."""
    from backends import get_backend
    from minppo_amd.train import save_model

    be = get_backend("hip")
    small = ["training.num_envs=64", "training.num_minibatches=2", "model.hidden_size=64"]
    ev = ["evaluation.num_envs=20", "evaluation.num_steps=8", "evaluation.record_envs=3"]
    tr = be.trainer(make_config(BASE, small + ev))
    tr.reset()
    tr.update()
    model = str(tmp_path / "model.pkl")
    save_model(tr.params, model)
    mine = tr.evaluate()
    tr.close()
    outs = []
    for i in range(2):
        npz = str(tmp_path / f"traj{i}.npz")
        p = subprocess.run([sys.executable, "-m", "minppo_amd.cli", "evaluate", "stompy_pro", *small, *ev, f"inference.model_path={model}", f"evaluation.trajectory_path={npz}"],
                           capture_output=True, text=True, cwd=str(ROOT), timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        line = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(line) == 1
        outs.append((json.loads(line[0]), dict(np.load(npz))))
    (s0, z0), (s1, z1) = outs
    assert s0 == s1 and s0["steps"] == 160 and set(z0) == {"qpos", "qvel", "action", "reward", "done", "dt", "n_frames"}
    for k in ("qpos", "qvel", "action", "reward", "done"):
        assert z0[k].shape[:2] == (9, 3) and np.array_equal(_bits(z0[k]), _bits(z1[k])), k
        assert np.array_equal(_bits(z0[k]), _bits(mine.trajectory[k])), k
    assert z0["qpos"].shape[2] == 17 and z0["action"].shape[2] == 10 and float(z0["dt"]) == pytest.approx(0.002) and int(z0["n_frames"]) == 1
    want = {k: (None if isinstance(v, float) and not np.isfinite(v) else v) for k, v in mine.stats().items()}
    assert s0 == want
