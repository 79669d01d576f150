"""Everything the environment step does AFTER the solver, pinned at float32 rounding: the Euler update of qvel, the semi-implicit position
update, the quaternion integration of free and ball joints, the warm-start carry, the n_frames loop, and the reward / done / time epilogue.

Against the float64 oracle these are visible only through the stepped state, inside tolerances sized for the unconverged float32 solver
(qpos 2e-3, qvel 0.15 per frame, reward 1e-2: DESIGN.md section 5).  But all of it is a pure function of values the C ABI exposes - the
record's own qvel', mppo_physics_forward's qacc and qacc_euler, the records' com_x - so it is checked here with no solver envelope at all.
Every tolerance in this file is bit-equality or one of two derived forms (tests/physics_harness.py):
  position  max(4 x |float32 reference - float64 reference| on the same inputs, 2^-22 max(1, |q|)) per entry   (position_bound)
  reward    64 x 2^-24 x the sum of the weighted terms' magnitudes per environment                             (reward_from_records)
Before any kernel is looked at, the float64 reference alone must tell three subtly wrong integrators from the right one by 100 x the
position bound (test_wrong_integrators_separate): the states (physics_harness.fast_states) are what makes the checks bite.

The largest errors measured per robot and backend (emulator, C++ twin, MI355X) are in DESIGN.md section 5, "After the solver"; every test prints its own.

The C++ twin runs the checks that need no probe, on the models it accepts; that it refuses the others (equalities, ball joints) is asserted."""

import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from minppo_amd.model import compile_model, load_model
from oracle.env_oracle import metrics_step
from oracle.physics_oracle import Physics, PhysState
from physics_harness import (METRIC_TYPES, ULP32, KernelStepper, TwinStepper, fast_states, position_bound, probe, quaternion_joints, record_of, reward_from_records,
                             run_steps, wrong_integrators)

f32, f64 = np.float32, np.float64
GOLDEN = Path(__file__).parent / "golden"
WIDE = (-5.0, 50.0)  # a height window no episode ends in
# reward weights unlike the defaults, no two alike: exp_coefficient, subtraction_factor, (max_diff_norm per robot), w_ctrl_cost, w_original_pos, w_is_healthy, w_velocity
EXP_C, SUB_F, W_CTRL, W_POS, W_HEALTHY, W_VEL = 1.7, 0.3, 0.13, 3.1, 0.7, 1.9
FUZZ_SEEDS = (7, 0)  # tests/test_model_fuzz.py::random_model: together a slide joint and a second free tree (asserted below)
N_ENVS = 4  # (one wave of the kernel)


def _fuzz(seed):
    from test_model_fuzz import random_model

    return compile_model(random_model(seed))


ROBOTS = {
    "synth_stompy_pro": lambda: load_model("synth_stompy_pro"),
    "synth_stompy_full": lambda: load_model("synth_stompy_full"),
    "synth_ball": lambda: load_model("synth_ball"),
    "ball_humanoid": lambda: load_model(str(GOLDEN / "ball_joints" / "ball_humanoid.xml")),
    "ball_chain": lambda: load_model(str(GOLDEN / "ball_joints" / "ball_chain.xml")),
    "fourbar_biped": lambda: load_model(str(GOLDEN / "equality" / "fourbar_biped.xml")),
    "hands_humanoid": lambda: load_model(str(GOLDEN / "many_dofs" / "hands_humanoid.xml")),
    "export_biped": lambda: load_model(str(GOLDEN / "export_biped" / "robot.xml")),  # (per-environment matrices in global memory)
    "random_a": lambda: _fuzz(FUZZ_SEEDS[0]),
    "random_b": lambda: _fuzz(FUZZ_SEEDS[1]),
}
SEEDS = {name: 20 + k for k, name in enumerate(ROBOTS)}  # (no environment of these is reset by the NaN guard on the emulator: asserted)
# the C++ twin reads no equality section and has no ball joint: it refuses these models (asserted where the twin's tests meet them)
TWIN_REFUSES = {"ball_humanoid", "ball_chain", "fourbar_biped", "hands_humanoid"}
_MODELS = {}


def _model(robot):
    if robot not in _MODELS:
        _MODELS[robot] = ROBOTS[robot]()
    return _MODELS[robot]


def _states(robot):
    cm = _model(robot)
    N = 8 if robot == "synth_ball" else N_ENVS   # (more balls: single contacts that six CG iterations nearly solve - see test_integrator_isolated)
    qpos, qvel, ctrl, warm = fast_states(cm, N, SEEDS[robot])
    if robot == "synth_ball":  # half of the balls 2 - 40 mm inside the ground: a constraint for the solver (the others fall freely)
        qpos[N // 2:, 2] = np.linspace(0.098, 0.06, N - N // 2)
    return cm, qpos, qvel, ctrl, warm


def _hand_records(robot, dims):
    """Hand-written records of the robot's fast states: start times 0 and 123.456 alternate, com_x is any number."""
    cm, qpos, qvel, ctrl, warm = _states(robot)
    N = qpos.shape[0]
    time = np.where(np.arange(N) % 2 == 0, 0.0, 123.456).astype(f32)
    com_x = np.linspace(-0.3, 0.4, N).astype(f32)
    return cm, record_of(dims, cm, qpos, qvel, warm, com_x, time), (qpos, qvel, ctrl, warm)


def _rc(window=WIDE, max_diff_norm=0.5):
    return (window[0], window[1], EXP_C, SUB_F, max_diff_norm, W_CTRL, W_POS, W_HEALTHY, W_VEL)


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _twin(robot):
    """The twin's stepper - or None, for a model the twin must refuse."""
    if robot in TWIN_REFUSES:
        with pytest.raises(ValueError, match="refused the model blob"):
            TwinStepper(_model(robot))
        return None
    return TwinStepper(_model(robot))


def _fields(cm, dims):
    nq, nv, O, OP = cm.nq, cm.nv, dims.obs_dim, dims.obs_pad
    return nq, nv, O, OP


def test_fuzz_robots_hold_a_slide_joint_and_a_second_free_tree():
    from minppo_amd.model import JNT_FREE, JNT_SLIDE

    types = [np.asarray(_model(r).t["jnt_type"]) for r in ("random_a", "random_b")]
    assert any((t == JNT_SLIDE).any() for t in types) and any((t == JNT_FREE).sum() >= 2 for t in types)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the states: from the float64 reference alone, a wrong integrator is 100 bounds away
# ---------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("robot", list(ROBOTS))
def test_wrong_integrators_separate(robot):
    """The states of this file are fast enough: |w| h in [0.1, 0.5] on every quaternion joint, |v| h in [0.01, 0.1] elsewhere (asserted), and
    each of three wrong position updates - quaternion multiplied on the wrong side, first-order quaternion update, old velocity - moves
    some qpos entry of the float64 reference by at least 100 x the bound the kernel is held to.  A robot without a quaternion joint
    has no case for the first two."""
    cm, qpos, qvel, ctrl, warm = _states(robot)
    N, h = qpos.shape[0], float(f32(cm.t["timestep"]))
    qj = quaternion_joints(cm)
    ang = np.zeros(cm.nv, bool)
    for qa, da in qj:
        ang[da:da + 3] = True
        wh = np.linalg.norm(qvel[:, da:da + 3].astype(f64), axis=1) * h
        assert (wh[0] == 0) and (wh[1:] >= 0.0999).all() and (wh[1:] <= 0.5001).all(), (robot, wh)
        n1 = np.linalg.norm(qpos[1, qa:qa + 4].astype(f64))
        assert 5e-4 < abs(n1 - 1) < 2e-3, (robot, n1)
    vh = np.abs(qvel[:, ~ang].astype(f64)) * h
    assert (vh >= 0.00999).all() and (vh <= 0.10001).all(), (robot, vh.min(), vh.max())
    d = PhysState(qpos=qpos.astype(f64), qvel=qvel.astype(f64), ctrl=ctrl.astype(f64), qacc_warmstart=warm.astype(f64), time=np.zeros(N))
    ph = Physics(cm.t)
    ph.forward(d)
    ph.euler(d)
    v_new = d.qvel.astype(f32)
    assert np.isfinite(v_new).all(), robot
    ref, bound = position_bound(cm, qpos, v_new)
    for name, wrong in wrong_integrators(cm, qpos, qvel, v_new).items():
        if wrong is None:
            assert not qj, robot
            continue
        ratio = (np.abs(wrong - ref) / bound).max()
        assert ratio >= 100.0, (robot, name, ratio)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the integrator, isolated
# ---------------------------------------------------------------------------------------------------------------------------------------


def _check_positions(st, robot, rec0, rec1, done, what):
    """qpos', quaternion norms, time and padding of a one-frame step from the record's own qvel' -> the largest position error / bound, in bounds."""
    cm, dims = st.cm, st.dims
    nq, nv, O, OP = _fields(cm, dims)
    ok = done == 0
    assert np.mean(~ok) <= 0.10, (what, robot, done)
    if st.name != "hip":
        assert ok.all(), (what, robot, done)   # (the seeds were chosen so)
    assert np.isfinite(rec1[ok]).all(), (what, robot)
    v_new = rec1[:, nq:nq + nv]
    ref, bound = position_bound(cm, rec0[:, :nq], v_new)
    err = np.abs(rec1[:, :nq].astype(f64) - ref)
    assert (err[ok] <= bound[ok]).all(), (what, robot, "qpos'", (err / bound)[ok].max(), err[ok].max())
    for qa, _ in quaternion_joints(cm):
        nrm = np.linalg.norm(rec1[ok, qa:qa + 4].astype(f64), axis=1)
        assert np.abs(nrm - 1).max() <= 2.0 ** -22, (what, robot, "norm of the quaternion at", qa, np.abs(nrm - 1).max())
    h = f32(cm.t["timestep"])
    assert _bits(rec1[ok, OP + nv + 1], (rec0[ok, OP + nv + 1] + h).astype(f32)), (what, robot, "time")
    assert (rec1[ok, O:OP] == 0).all() and (rec1[ok, OP + nv + 2:] == 0).all(), (what, robot, "padding")
    return float((err / bound)[ok].max()), float(err[ok].max())


@pytest.mark.parametrize("robot", list(ROBOTS))
def test_integrator_isolated(be, robot):
    """One env_step (n_frames = 1) from a hand-written record and mppo_physics_forward on the same qpos, qvel, ctrl and warm start: the new
    warm start IS the probe's qacc and qvel' IS float32(qvel + float32(h) qacc_euler), bit for bit; qpos' is the float64 integration of
    the record's own qvel' within the position bound; quaternions of norm 1 within 2^-22; time' = float32(time + float32(h)) from 0 and
    from 123.456; the padding zero; the observation the record as it was.  And the velocity check bites: advancing qvel with the
    solver's qacc instead of qacc_euler moves some dof by more than 100 float32 ulp (damping, or a solver that has not converged)."""
    st = KernelStepper(be, _model(robot))
    cm, rec0, (qpos, qvel, ctrl, warm) = _hand_records(robot, st.dims)
    nq, nv, O, OP = _fields(cm, st.dims)
    rec1, obs, rew, done = st.step(rec0, ctrl, 1, _rc())
    got = probe(be, st.h, cm, qpos, qvel, ctrl, warm)
    st.close()
    ratio, err = _check_positions(st, robot, rec0, rec1, done, be.name)
    print(f"[step_exact] {be.name} {robot}: max |qpos' - float64| = {err:.3g} ({ratio:.3f} of its bound)")
    ok = done == 0
    assert _bits(obs[:, :OP], rec0[:, :OP]), (robot, "observation")
    h = f32(cm.t["timestep"])
    v_want = (qvel + h * got["qacc_euler"]).astype(f32)
    v_mutant = (qvel + h * got["qacc"]).astype(f32)
    sep = np.abs(v_mutant.astype(f64) - v_want.astype(f64)) / np.spacing(np.maximum(np.abs(v_want), f32(1e-3))).astype(f64)   # (a dof at rest counts as 1e-3)
    print(f"[step_exact] {be.name} {robot}: qvel' with the solver's qacc is {sep[ok].max():.3g} float32 ulp away")
    assert sep[ok].max() >= 100.0, (robot, "qacc and qacc_euler are too close for the velocity check to tell them apart", sep[ok].max())
    assert _bits(rec1[ok, OP:OP + nv], got["qacc"][ok]), (robot, "warm start", np.abs(rec1[ok, OP:OP + nv] - got["qacc"][ok]).max())
    assert _bits(rec1[ok, nq:nq + nv], v_want[ok]), (robot, "qvel'", np.abs(rec1[ok, nq:nq + nv] - v_want[ok]).max())


@pytest.mark.parametrize("robot", list(ROBOTS))
def test_integrator_positions_on_the_twin(robot):
    """The position, norm, time and padding checks of test_integrator_isolated on the C++ twin (they need no probe)."""
    st = _twin(robot)
    if st is None:
        return
    cm, rec0, (qpos, qvel, ctrl, warm) = _hand_records(robot, st.dims)
    rec1, obs, rew, done = st.step(rec0, ctrl, 1, _rc())
    st.close()
    ratio, err = _check_positions(st, robot, rec0, rec1, done, "twin")
    print(f"[step_exact] twin {robot}: max |qpos' - float64| = {err:.3g} ({ratio:.3f} of its bound)")
    assert _bits(obs[:, :st.dims.obs_pad], rec0[:, :st.dims.obs_pad]), (robot, "observation")


# ---------------------------------------------------------------------------------------------------------------------------------------
# frames compose
# ---------------------------------------------------------------------------------------------------------------------------------------


def _check_frames(st, robot):
    cm, dims = st.cm, st.dims
    nq, nv, O, OP = _fields(cm, dims)
    _, rec_hand, (qpos, qvel, ctrl, warm) = _hand_records(robot, dims)
    rc = _rc()
    N = rec_hand.shape[0]
    other = np.roll(ctrl, 1, axis=0) * f32(-0.5) + f32(0.25)   # a different action
    # a first step fills the record's c-vals and qfrc_actuator (the observation of the next call)
    rec0, _, _, d0 = st.step(rec_hand, ctrl, 1, rc)
    assert not d0.any(), (st.name, robot)
    h = f32(cm.t["timestep"])
    for k in (2, 3, 5):
        rec_k, obs_k, rew_k, done_k = st.step(rec0, ctrl, k, rc)
        r = rec0
        for _ in range(k):
            r, _, _, d1 = st.step(r, ctrl, 1, rc)
            assert not d1.any(), (st.name, robot, k)
        assert not done_k.any(), (st.name, robot, k)
        diff = np.argwhere(rec_k.view(np.uint32) != r.view(np.uint32))
        assert diff.size == 0, (st.name, robot, k, "the k-frame record is not k one-frame records", diff[:6].tolist(), OP + nv + 1)
        assert _bits(obs_k[:, :OP], rec0[:, :OP]), (st.name, robot, k, "observation")
        # time' = time + k h by k float32 additions of h, as the reference's k mjx.step calls make them (the bit-equality above): k roundings of
        # half an ulp each from the exact sum (k h rounded once and added would be one rounding - and another record, by a bit, at large times)
        t_exact = rec0[:, OP + nv + 1].astype(f64) + k * float(h)
        t_got = rec_k[:, OP + nv + 1]
        assert (np.abs(t_got.astype(f64) - t_exact) <= k * 0.5 * np.spacing(np.maximum(t_got, t_exact.astype(f32)))).all(), (st.name, robot, k, "time")
        # the velocity term of the reward spans k h: recomputed from the records' own com_x
        want, bound, _ = reward_from_records(cm, rec0, rec_k, ctrl, rc, k, dims)
        assert (np.abs(rew_k.astype(f64) - want) <= bound).all(), (st.name, robot, k, "reward", np.abs(rew_k - want).max(), bound.min())
        if cm.nu and k == 3:   # frames 2 .. k use the call's action: with another action the result differs already in qvel'
            rec_o, _, _, _ = st.step(rec0, other, k, rc)
            r1, _, _, _ = st.step(rec0, other, 1, rc)
            for _ in range(k - 1):
                r1, _, _, _ = st.step(r1, other, 1, rc)
            assert _bits(rec_o, r1), (st.name, robot, k, "second action")
            assert (rec_o[:, nq:nq + nv] != rec_k[:, nq:nq + nv]).any(), (st.name, robot, k, "the action does not reach qvel'")


@pytest.mark.parametrize("robot", list(ROBOTS))
def test_frames_compose(be, robot):
    """env_step(n_frames = k), k in {2, 3, 5}, IS k calls with n_frames = 1 on the same action - the record bit for bit; its observation is the
    record from before the first frame (qpos, qvel, c-vals, qfrc_actuator); time advances by k h; the reward's velocity term spans k h; no
    episode ends.  Frames 2 .. k re-read the action from storage the solver overwrote: a second action gives k one-frame calls of ITS own."""
    st = KernelStepper(be, _model(robot))
    try:
        _check_frames(st, robot)
    finally:
        st.close()


@pytest.mark.parametrize("robot", list(ROBOTS))
def test_frames_compose_on_the_twin(robot):
    st = _twin(robot)
    if st is None:
        return
    try:
        _check_frames(st, robot)
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the epilogue from the records
# ---------------------------------------------------------------------------------------------------------------------------------------


def _check_epilogue(st, robot):
    cm, dims = st.cm, st.dims
    nq, nv, O, OP = _fields(cm, dims)
    _, rec_hand, (qpos, qvel, ctrl, warm) = _hand_records(robot, dims)
    N = rec_hand.shape[0]
    rec0, _, _, d0 = st.step(rec_hand, ctrl, 1, _rc())   # (c-vals in the record; the stepped pose is further from qpos0 than the hand-written one)
    assert not d0.any()
    p0 = np.linalg.norm(np.asarray(cm.t["qpos0"], f32).astype(f64)[None] - rec0[:, :nq].astype(f64), axis=1)
    mdn = float(f32(np.median(p0)))   # clips half of the environments
    rc = _rc(max_diff_norm=mdn)
    worst = 0.0
    for k in (1, 3):
        rec1, obs, rew, done = st.step(rec0, ctrl, k, rc)
        assert not done.any(), (st.name, robot, k)
        want, bound, clipped = reward_from_records(cm, rec0, rec1, ctrl, rc, k, dims)
        assert clipped.any() and not clipped.all(), (st.name, robot, p0, mdn)
        err = np.abs(rew.astype(f64) - want)
        worst = max(worst, float((err / (bound / 64.0)).max()))
        assert (err <= bound).all(), (st.name, robot, k, "reward", (err / bound).max())
    print(f"[step_exact] {st.name} {robot}: max |reward - float64| = {worst:.2f} x 2^-24 x sum |terms| (allowed 64)")

    # ---- the thresholds: done is strict on both sides (post-step z), healthy inclusive at both ends (pre-step z) ----
    rec1, _, rew_wide, _ = st.step(rec0, ctrl, 1, rc)
    z0, z1 = rec0[:, 2].copy(), rec1[:, 2].copy()
    lo, hi = int(np.argmin(z1)), int(np.argmax(z1))
    assert (z1 != z1[lo]).sum() == N - 1 and (z1 != z1[hi]).sum() == N - 1, (robot, z1)   # (no ties: the other environments stay inside)
    ninf, pinf = f32(-np.inf), f32(np.inf)
    rng = np.random.default_rng(5)
    for window, i, ends in (((z1[lo], WIDE[1]), lo, True), ((np.nextafter(z1[lo], ninf), WIDE[1]), lo, False),
                            ((WIDE[0], z1[hi]), hi, True), ((WIDE[0], np.nextafter(z1[hi], pinf)), hi, False)):
        met = {kk: (rng.integers(1, 50, N).astype(t) if t != f32 else rng.uniform(-3, 3, N).astype(f32)) for kk, t in METRIC_TYPES.items()}
        met0 = {kk: v.copy() for kk, v in met.items()}
        rc_w = _rc(window=tuple(float(x) for x in window), max_diff_norm=mdn)
        rec_w, obs_w, rew_w, done_w = st.step(rec0, ctrl, 1, rc_w, metrics=met)
        want_done = np.zeros(N, np.uint8)
        want_done[i] = 1 if ends else 0
        assert (done_w == want_done).all(), (st.name, robot, window, i, done_w)
        want_w, bound_w, _ = reward_from_records(cm, rec0, rec1, ctrl, rc_w, 1, dims)   # (healthy reads the window too, at the pre-step z)
        assert (np.abs(rew_w.astype(f64) - want_w) <= bound_w).all(), (st.name, robot, window, "reward")
        keep = want_done == 0
        assert _bits(rec_w[keep], rec1[keep]) and _bits(obs_w[keep, :OP], rec0[keep, :OP]), (st.name, robot, window)
        if ends:   # the ended episode: the reset record, bit for bit, as record and as observation
            assert _bits(rec_w[i], st.reset_rec) and _bits(obs_w[i, :OP], st.reset_rec[:OP]), (st.name, robot, "reset record")
        m_want = metrics_step(met0, rew_w, done_w, f32)
        for kk, t in METRIC_TYPES.items():
            assert np.array_equal(np.asarray(met[kk]).astype(t), np.asarray(m_want[kk]).astype(t)), (st.name, robot, kk, met[kk], m_want[kk])
    lo, hi = int(np.argmin(z0)), int(np.argmax(z0))
    assert (z0 != z0[lo]).sum() == N - 1 and (z0 != z0[hi]).sum() == N - 1, (robot, z0)
    for inside, outside, i in (((z0[lo], WIDE[1]), (np.nextafter(z0[lo], pinf), WIDE[1]), lo), ((WIDE[0], z0[hi]), (WIDE[0], np.nextafter(z0[hi], ninf)), hi)):
        r_in = st.step(rec0, ctrl, 1, _rc(window=tuple(float(x) for x in inside), max_diff_norm=mdn))[2]
        r_out = st.step(rec0, ctrl, 1, _rc(window=tuple(float(x) for x in outside), max_diff_norm=mdn))[2]
        assert _bits(r_in, rew_wide), (st.name, robot, "healthy at the end of the window itself", inside)
        others = np.arange(N) != i
        assert _bits(r_out[others], rew_wide[others]), (st.name, robot, outside)
        _, bound, _ = reward_from_records(cm, rec0, rec1, ctrl, rc, 1, dims)
        assert abs((float(r_in[i]) - float(r_out[i])) - float(f32(W_HEALTHY))) <= bound[i], (st.name, robot, r_in[i], r_out[i])


@pytest.mark.parametrize("robot", list(ROBOTS))
def test_epilogue_from_the_records(be, robot):
    """The reward recomputed in float64 from the pre-step record (|qpos0 - qpos| over all of qpos, z, com_x), the action and the post-step
    record's com_x, n_frames 1 and 3, under weights unlike the defaults and a max_diff_norm that clips some environments and not others:
    within 64 x 2^-24 of the sum of the weighted terms' magnitudes.  The height window through the kernel's own comparisons: done strict on
    both sides at the post-step z and its float32 neighbours, healthy inclusive at both ends at the pre-step z, every other
    environment untouched; an ended episode's record and observation are the reset record bit for bit, and the metrics roll over
    as oracle.env_oracle.metrics_step says."""
    st = KernelStepper(be, _model(robot))
    try:
        _check_epilogue(st, robot)
    finally:
        st.close()


@pytest.mark.parametrize("robot", list(ROBOTS))
def test_epilogue_from_the_records_on_the_twin(robot):
    st = _twin(robot)
    if st is None:
        return
    try:
        _check_epilogue(st, robot)
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# full size on the GPU
# ---------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("model,N", [("synth_stompy_pro", 4096), ("synth_stompy_full", 8192)])
def test_free_running_steps_are_exact_at_full_size(model, N):
    """40 free-running steps under random actions and the default reward window: for every consecutive pair of records whose episode did not
    end, the position check and the time check of test_integrator_isolated and the reward recomputation of
    test_epilogue_from_the_records - every workgroup placement, the auto-reset path at scale.  At least 90 % of the pairs are checkable."""
    import torch

    from minppo_amd import _native as nat

    cm = load_model(model)
    lib = nat.load()
    blob = np.frombuffer(cm.to_blob(), np.uint8)
    dblob = torch.from_numpy(blob.copy()).cuda()
    hdl = C.c_void_p()
    lib.model_open(blob.ctypes.data, blob.size, dblob.data_ptr(), C.byref(hdl))
    dims = nat.ModelDims()
    lib.model_get_dims(hdl, C.byref(dims))
    start, actions = [], []
    out = run_steps(lib, hdl, dims, N, 40, torch, seed=2, start=start, actions=actions)
    lib.model_close(hdl)
    nq, nv, O, OP = _fields(cm, dims)
    rc = (-0.2, 2.0, 2.0, 0.2, 0.5, 0.1, 4.0, 1.0, 1.25)   # (run_steps')
    h = f32(cm.t["timestep"])
    prev, checked, worst_q, worst_r = start[0], 0, 0.0, 0.0
    for t, (rec, obs, rew, done) in enumerate(out):
        ok = done == 0
        checked += int(ok.sum())
        ref, bound = position_bound(cm, prev[ok, :nq], rec[ok, nq:nq + nv])
        err = np.abs(rec[ok, :nq].astype(f64) - ref)
        worst_q = max(worst_q, float((err / bound).max()))
        assert (err <= bound).all(), (t, "qpos'", (err / bound).max())
        assert _bits(rec[ok, OP + nv + 1], (prev[ok, OP + nv + 1] + h).astype(f32)), (t, "time")
        want, rbound, _ = reward_from_records(cm, prev[ok], rec[ok], actions[t][ok], rc, 1, dims)
        rerr = np.abs(rew[ok].astype(f64) - want)
        worst_r = max(worst_r, float((rerr / (rbound / 64.0)).max()))
        assert (rerr <= rbound).all(), (t, "reward", (rerr / rbound).max())
        assert _bits(obs[:, :OP][ok], prev[ok, :OP]), (t, "observation")
        prev = rec
    print(f"[step_exact] hip {model} N={N}: {checked} pairs, max position error {worst_q:.3f} of its bound, reward {worst_r:.2f} x 2^-24 x sum |terms| (allowed 64)")
    assert checked >= 0.9 * 40 * N, checked


# ---------------------------------------------------------------------------------------------------------------------------------------
# the engine passes n_frames through
# ---------------------------------------------------------------------------------------------------------------------------------------


def test_engine_rollout_with_two_frames_is_env_step_with_two_frames(be):
    """A Trainer with environment.n_frames = 2: the rollout's rewards, done flags and final state records equal, bit for bit, stand-alone
    env_step(n_frames = 2) calls replayed from the reset record with the engine's own actions."""
    from minppo_amd.config import make_config
    from minppo_amd.train import reward_cfg

    small = ["training.num_envs=8", "training.num_steps=4", "rl.num_env_steps=4", "training.num_minibatches=2", "model.hidden_size=32"] if be.name == "emu" else \
            ["training.num_envs=256", "training.num_minibatches=8"]
    cfg = make_config({"kscale_id": "5eb3cb7f23232298", "visualization": {"camera_name": "track"}},
                      [*small, "training.update_epochs=2", "training.total_timesteps=100000000", "environment.n_frames=2"])
    tr = be.trainer(cfg, external_random=True, use_graph=False)
    tr.reset()
    N, T, A = tr.N, tr.T, tr.A
    be.put(tr.region("noise", (T, N, A)), np.random.default_rng(0).standard_normal((T, N, A)).astype(f32))
    tr.rollout()
    tr._sync()
    tj = {k: be.host(v).copy() for k, v in tr.traj().items()}
    final = be.host(tr.region("state", (N, tr.dims.rec_dim))).copy()
    r = reward_cfg(cfg)
    rc = tuple(getattr(r, n) for n, _ in r._fields_)
    st = KernelStepper(be, tr.cm)
    rec = np.tile(st.reset_rec, (N, 1))
    assert _bits(tj["obs"][0], rec[:, :tr.OP])
    h2, t_want = f32(f32(tr.cm.t["timestep"]) * f32(2)), np.zeros(N, f32)
    for t in range(T):
        rec, obs, rew, done = st.step(rec, tj["action"][t], 2, rc)
        t_want = np.where(done != 0, f32(0), (t_want + h2).astype(f32)).astype(f32)
        assert _bits(obs, tj["obs"][t + 1]), t
        assert _bits(rew, tj["reward"][t]), (t, np.abs(rew - tj["reward"][t]).max())
        assert np.array_equal(done.astype(bool), tj["done"][t].astype(bool)), t
    assert _bits(rec, final)
    # (and it is two frames that ran: the time advanced by 2 h per step where no episode ended)
    assert not tj["done"].all() and _bits(final[:, tr.OP + tr.cm.nv + 1], t_want)
    st.close()
    tr.close()
