"""Random pushes: an external wrench in the environment kernel (csrc/k_physics.hip), its stateless draw (csrc/push.h, k_push.hip), the engine
(`mppo_engine_set_push`), the evaluator (`mppo_evaluate_push`) and the Python surface (`environment.push_*`, `HumanoidEnv.step(xfrc=)`).

1. the draw, bit for bit against `jaxrng.push_wrench_philox`        6. the draw inside the kernel equals mppo_push_fill + mppo_env_step_xfrc
2. the forward probe against the float64 oracle under the wrench    7. a pushed evaluation leaves the unpushed one exactly where the first push acts
3. known answers (a pushed ball, a twisted brick)                   8. the engine: off is off, graph = eager, checkpoint / resume, call order
4. env steps against EnvOracle under the wrench                     9. config keys, HumanoidEnv, the command line
5. specialised / run-time-sized / out-of-LDS kernels, bit for bit

The reference of 2 and 4 is the oracle with `PushedPhysics` below: `fwd_acceleration` adds jacp(xipos[b], b)^T f + jacr^T tau to qfrc_smooth - MuJoCo's
mj_xfrcAccumulate through the point Jacobian, NOT the kernel's cdof form.  Sizes: N = 37 for the draws, 5 / 7 for the physics - no multiple of the four
environments of a wave."""

import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import physics_harness as ph
from minppo_amd import _native as nat
from minppo_amd import jaxrng
from minppo_amd import model as M
from minppo_amd.config import make_config
from minppo_amd.model import JNT_FREE, JNT_HINGE, compile_model, load_model
from minppo_amd.train import init_flat_params, reward_cfg
from oracle.env_oracle import EnvOracle, RewardCfg
from oracle.physics_oracle import Physics, PhysState
from physics_harness import GOLDEN, METRIC_TYPES, SMOOTH_TOL, pack

f32, f64 = np.float32, np.float64
ROOT = Path(__file__).resolve().parent.parent
BASE = {"kscale_id": "5eb3cb7f23232298", "visualization": {"camera_name": "track"}}
SEED = 5
F, I, D = 40.0, 7, 3
RC = (-0.2, 2.0, 2.0, 0.2, 0.5, 0.1, 4.0, 1.0, 1.25)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _pcfg(body=1, interval=I, duration=D, rank=0, force=F, seed=SEED):
    return nat.PushCfg(body=body, interval=interval, duration=duration, rank=rank, force=force, seed=seed)


def _fill(be, p, N, step=0, counter=None, mul=0):
    out = be.full((N, 6), np.nan)
    ctr = be.arr(np.array([counter], np.int32)) if counter is not None else None
    be.lib.push_fill(C.byref(p), N, be.ptr(ctr), mul, step, be.ptr(out), be.stream)
    be.sync()
    return be.host(out).copy()


class PushedPhysics(Physics):
    """The oracle under `xfrc` [N, 6] (force, torque; world axes) at the centre of mass of `body`: qfrc_smooth += jacp(xipos[b], b)^T f + jacr(b)^T tau."""

    body, xfrc = 1, None

    def fwd_acceleration(self, d):
        super().fwd_acceleration(d)
        if self.xfrc is None or self.xfrc.shape[0] != d.qpos.shape[0]:  # (the one-environment reset state of EnvOracle is never pushed)
            return
        x = self.xfrc.astype(self.dtype)
        q = np.einsum("nkv,nk->nv", self.jacp(d, d.xipos[:, self.body], self.body), x[:, :3])
        dof = self.body_lastdof[self.body]
        while dof >= 0:  # the rotational Jacobian's column of an ancestor dof is its cdof's angular half
            q[:, dof] += np.einsum("nk,nk->n", d.cdof[:, dof, :3], x[:, 3:])
            dof = self.t["dof_parentid"][dof]
        d["qfrc_smooth"] = d.qfrc_smooth + q
        d["qacc_smooth"] = self.solve_m(d, d.qfrc_smooth)


# ---- 1: the draw ----------------------------------------------------------------------------------------------------------------------------------------


def test_fill_equals_the_host_restatement(be):
    N = 37
    p = _pcfg()
    rows = np.stack([_fill(be, p, N, s) for s in range(21)])
    want = np.stack([jaxrng.push_wrench_philox(SEED, 0, s, N, F, I, D) for s in range(21)])
    assert np.array_equal(_bits(rows), _bits(want))
    # a step read from a device counter: 5 * 10 + 3
    assert np.array_equal(_bits(_fill(be, p, N, 3, counter=5, mul=10)), _bits(jaxrng.push_wrench_philox(SEED, 0, 53, N, F, I, D)))
    on = (rows[:, :, :2] != 0).any(2)
    for s in range(21 - I + 1):  # exactly D of any I consecutive steps
        assert (on[s:s + I].sum(0) == D).all(), s
    assert (rows[~on] == 0).all() and (_bits(rows[~on]) == 0).all()  # exact zeros (no -0)
    assert (rows[:, :, 2:] == 0).all() and (_bits(rows[:, :, 2:]) == 0).all()
    assert np.abs(rows[:, :, :2]).max() <= F and np.abs(rows[:, :, :2]).max() > 0.5 * F
    assert len({tuple(on[:I, n]) for n in range(N)}) > 1  # the environments are out of phase
    # a force holds for its whole window
    for n in range(N):
        starts = [s for s in range(1, 21 - D + 1) if on[s, n] and not on[s - 1, n]]
        for s in starts:
            assert all(np.array_equal(rows[s, n], rows[s + k, n]) for k in range(D)), (n, s)
    # another seed, another rank: another draw
    assert not np.array_equal(_fill(be, _pcfg(seed=SEED + 1), N, 0), rows[0]) and not np.array_equal(_fill(be, _pcfg(rank=1), N, 0), rows[0])
    assert np.array_equal(_bits(_fill(be, _pcfg(rank=1), N, 4)), _bits(jaxrng.push_wrench_philox(SEED, 1, 4, N, F, I, D)))
    # D = I: always pushed
    always = np.stack([_fill(be, _pcfg(duration=I), N, s) for s in range(I + 2)])
    assert (always[:, :, :2] != 0).any(2).all()
    assert np.array_equal(_bits(always[3]), _bits(jaxrng.push_wrench_philox(SEED, 0, 3, N, F, I, I)))
    # force 0: zeros
    assert (_bits(_fill(be, _pcfg(force=0.0), N, 2)) == 0).all()


def test_fill_refuses_bad_configurations(be):
    out = be.zeros((4, 6))
    f = be.lib._fn["mppo_push_fill"]
    for bad, word in ((_pcfg(force=-1.0), "negative"), (_pcfg(force=float("nan")), "negative"), (_pcfg(interval=0), "interval"), (_pcfg(duration=0), "duration"),
                      (_pcfg(duration=I + 1), "duration"), (_pcfg(rank=300), "rank")):
        assert f(C.byref(bad), 4, 0, 0, 0, be.ptr(out), be.stream) != 0 and word in be.lib.last_error(), word
    with pytest.raises(ValueError):
        jaxrng.push_wrench_philox(SEED, 0, 0, 4, F, I, I + 1)


# ---- 2: the forward probe under a wrench against the pushed oracle ------------------------------------------------------------------------------------


def _many_bodies():
    """A free root and 70 one-hinge bodies in three interleaved chains: 72 bodies (two words per body in body_subtree_mask), 76 dofs; the deepest bodies
    have the highest ids."""
    rng = np.random.default_rng(9)
    bodies = [M.BodySpec("root", "world", mass=2.0, inertia=(0.02, 0.02, 0.02), joints=[M.JointSpec("free", JNT_FREE)])]
    for k in range(70):
        bodies.append(M.BodySpec(f"b{k}", "root" if k < 3 else f"b{k - 3}", pos=tuple(0.05 * rng.normal(size=3)), mass=0.2, inertia=(2e-4, 3e-4, 4e-4),
                                 ipos=tuple(0.01 * rng.normal(size=3)),
                                 joints=[M.JointSpec(f"j{k}", JNT_HINGE, axis=tuple(rng.normal(size=3)), range=(-0.5, 0.5), damping=0.2, armature=0.01)]))
    return compile_model(M.ModelSpec("many_bodies", bodies, [M.ActuatorSpec(f"j{k}", kp=2.0) for k in (0, 35, 69)], free_root_z=0.6))


ROBOTS = {"pro": lambda: load_model("synth_stompy_pro"),                                   # a library instantiation
          "hand_leg": lambda: load_model(str(GOLDEN / "hand_leg.xml")),                    # the run-time-sized kernel
          "ball_humanoid": lambda: load_model(str(GOLDEN / "ball_joints" / "ball_humanoid.xml")),
          "export_biped": lambda: load_model(str(GOLDEN / "export_biped" / "robot.xml")),  # matrices in global memory
          "many_bodies": _many_bodies}
_CM = {}


def _cm(which):
    if which not in _CM:
        _CM[which] = ROBOTS[which]()
    return _CM[which]


def _push_bodies(cm):
    """The root, the deepest body and a body half way up its chain; beyond 64 bodies also a non-leaf body of the second word."""
    parent = [int(x) for x in cm.t["body_parent"]]
    depth = [0] * cm.nbody
    for b in range(1, cm.nbody):
        depth[b] = depth[parent[b]] + 1
    deepest = int(np.argmax(depth))
    mid = deepest
    while depth[mid] > (depth[deepest] + 1) // 2:
        mid = parent[mid]
    out = [1, deepest, mid]
    if cm.nbody > 64:
        out.append(parent[parent[deepest]])
        assert deepest >= 64 and out[-1] >= 64
    return out


def _probe_x(be, h, cm, q32, body, xfrc):
    """ph.probe through mppo_physics_forward_xfrc (xfrc None: a null pointer)."""
    N = q32[0].shape[0]
    nv, nb, nefc = cm.nv, cm.nbody, max(cm.nefc, 1)
    shapes = dict(qM=(N, nv, nv), qfrc_bias=(N, nv), qfrc_passive=(N, nv), qfrc_actuator=(N, nv), qacc_smooth=(N, nv), efc_J=(N, nefc, nv), efc_D=(N, nefc),
                  efc_aref=(N, nefc), qacc=(N, nv), cinert=(N, nb, 10), cvel=(N, nb, 6), subtree_com1=(N,), xpos=(N, nb, 3), qacc_euler=(N, nv))
    out = {k: be.zeros(s) for k, s in shapes.items()}
    niter = be.zeros((N,), np.int32)
    d_in = [be.arr(x.astype(f32)) for x in q32]
    x = be.arr(xfrc.astype(f32)) if xfrc is not None else None
    pr = nat.ForwardProbe(**{k: be.ptr(v) for k, v in out.items()}, solver_niter=be.ptr(niter))
    be.lib.physics_forward_xfrc(h, N, be.ptr(d_in[0]), be.ptr(d_in[1]), be.ptr(d_in[2]) if cm.nu else 0, be.ptr(d_in[3]), C.byref(pr), body, be.ptr(x), be.stream)
    be.sync()
    res = {k: be.host(v).copy() for k, v in out.items()}
    res["niter"] = be.host(niter).copy()
    return res


def _oracle_smooth(cm, q32, body, xfrc):
    """qacc_smooth of the float64 oracle under the wrench (the forward pass up to fwd_acceleration: nothing after it feeds back)."""
    N = q32[0].shape[0]
    d = PhysState(qpos=q32[0].astype(f64), qvel=q32[1].astype(f64), ctrl=q32[2].astype(f64)[:, :cm.nu], qacc_warmstart=q32[3].astype(f64), time=np.zeros(N, f64))
    P = PushedPhysics(cm.t, f64)
    P.body, P.xfrc = body, None if xfrc is None else xfrc.astype(f64)
    P.kinematics(d); P.com_pos(d); P.crb(d); P.com_vel(d); P.passive(d); P.rne(d); P.fwd_actuation(d); P.fwd_acceleration(d)
    return d.qacc_smooth


@pytest.mark.parametrize("which", list(ROBOTS))
def test_forward_probe_follows_the_pushed_oracle(be, which):
    cm = _cm(which)
    N = 5
    rng = np.random.default_rng(21)
    qpos, qvel, ctrl = ph.random_states(cm, N, rng)
    q32 = [x.astype(f32) for x in (qpos, qvel, ctrl if cm.nu else np.zeros((N, 1)), np.zeros((N, cm.nv)))]
    h, dims, _keep = be.model(cm)
    plain = ph.probe(be, h, cm, *q32)
    be.sync()
    plain = {k: np.array(v) for k, v in plain.items()}
    # xfrc = NULL and an all-zero wrench: mppo_physics_forward, every output, bit for bit
    for body, x in ((0, None), (_push_bodies(cm)[1], np.zeros((N, 6), f32))):
        ph.assert_bit_equal(plain, _probe_x(be, h, cm, q32, body, x))
    ref0 = _oracle_smooth(cm, q32, 1, None)
    for body in _push_bodies(cm):
        x = np.concatenate([rng.uniform(-50, 50, (N, 3)), rng.uniform(-5, 5, (N, 3))], 1).astype(f32)
        got = _probe_x(be, h, cm, q32, body, x)
        ref = _oracle_smooth(cm, q32, body, x)
        scale = np.abs(ref).max() + 1e-6
        err = np.abs(got["qacc_smooth"] - ref).max() / scale
        print(f"{which} body {body}: qacc_smooth err {err:.3e} of scale {scale:.3e}; the wrench moves it by {np.abs(ref - ref0).max() / scale:.3e}")
        # (a kernel that ignored the wrench would be off by what the wrench does to the reference, less its own error: beyond the tolerance if that is two of them)
        assert np.abs(ref - ref0).max() > 2 * SMOOTH_TOL["qacc_smooth"] * scale
        assert err <= SMOOTH_TOL["qacc_smooth"], (which, body, err)
        for k in ("qM", "qfrc_bias", "qfrc_passive", "qfrc_actuator", "xpos", "cinert", "cvel"):
            assert np.array_equal(_bits(got[k]), _bits(plain[k])), (which, body, k)
        assert not np.array_equal(got["qacc_smooth"], plain["qacc_smooth"]) and not np.array_equal(got["qacc_euler"], plain["qacc_euler"])
    # a body the model does not have, the world body
    f = be.lib._fn["mppo_physics_forward_xfrc"]
    z = be.zeros((N, 6))
    d_in = [be.arr(a) for a in q32]
    pr = nat.ForwardProbe()
    for body in (0, cm.nbody, -1):
        assert f(h, N, be.ptr(d_in[0]), be.ptr(d_in[1]), be.ptr(d_in[2]) if cm.nu else 0, be.ptr(d_in[3]), C.byref(pr), body, be.ptr(z), be.stream) != 0
        assert "push body" in be.lib.last_error()
    be.lib.model_close(h)


# ---- 3: known answers ---------------------------------------------------------------------------------------------------------------------------------


def _stepper(be, cm, N, raise_z=0.0, upright=False):
    h, dims, keep = be.model(cm)
    OP, R = dims.obs_pad, dims.rec_dim
    state, reset_rec, obs = be.zeros((N, R)), be.zeros((R,)), be.zeros((N, OP))
    rew, done = be.zeros((N,)), be.zeros((N,), np.uint8)
    be.lib.env_reset(h, N, be.ptr(state), be.ptr(reset_rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), None, be.stream)
    be.sync()
    if raise_z:
        s = be.host(state).copy()
        s[:, 2] += raise_z
        if upright:  # (a free root's quaternion: body frame = world frame)
            s[:, 3:7] = [1.0, 0.0, 0.0, 0.0]
        be.put(state, s)
    rc = nat.RewardCfg(-0.2, 5.0, *RC[2:])
    nu = max(cm.nu, 1)
    act = be.zeros((N, nu))

    def step(body=1, xfrc=None, n_frames=1, action=None):
        a = act if action is None else be.arr(action.astype(f32))
        x = be.arr(xfrc.astype(f32)) if xfrc is not None else None
        be.lib.env_step_xfrc(h, N, n_frames, C.byref(rc), be.ptr(state), be.ptr(reset_rec), be.ptr(a), nu, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), None, body,
                             be.ptr(x), be.stream)
        be.sync()
        return be.host(state).copy()

    return h, dims, keep, step, (state, obs, rew, done)


def test_a_pushed_ball_follows_the_closed_form(be):
    """A free sphere in the air under f = (3, -1, 0): x_K = (f / m) h^2 K (K + 1) / 2 (semi-implicit Euler from rest), z the unpushed fall bit for bit.
    rtol 2e-6: test_free_fall_is_exact_semi_implicit_euler's, for the same chain of operations."""
    cm = load_model("synth_ball")
    N, K, hh = 3, 50, 0.002
    m = float(cm.t["body_mass"][1])
    f = np.array([3.0, -1.0, 0.0])
    x = np.tile(np.concatenate([f, np.zeros(3)]).astype(f32), (N, 1))
    h1, _, _k1, step1, _ = _stepper(be, cm, N)
    h0, _, _k0, step0, _ = _stepper(be, cm, N)
    for _ in range(K):
        s1, s0 = step1(1, x), step0(1, None)
    want = f / m * hh * hh * K * (K + 1) / 2
    print("x, y after 50 steps:", s1[0, :2], "closed form:", want[:2])
    assert abs(want[0] - 0.0153) < 5e-5 and abs(want[1] + 0.0051) < 5e-5  # (the float64 oracle's figures)
    np.testing.assert_allclose(s1[:, 0] - s0[:, 0], want[0], rtol=2e-6)
    np.testing.assert_allclose(s1[:, 1] - s0[:, 1], want[1], rtol=2e-6)
    assert np.array_equal(_bits(s1[:, 2]), _bits(s0[:, 2]))
    np.testing.assert_allclose(s1[:, 2], 0.5 - 9.81 * hh * hh * K * (K + 1) / 2, rtol=2e-6)
    be.lib.model_close(h1); be.lib.model_close(h0)


def test_a_torque_spins_a_brick_about_its_principal_axis(be):
    """A box at rest in the air, body frame = world frame, a torque about one principal axis: after one step w = h tau / I on that axis and nothing else turns."""
    cm = load_model("synth_brick")
    N, hh = 3, float(cm.t["timestep"])
    assert np.allclose(cm.t["body_iquat"][1], [1, 0, 0, 0]) and len(set(np.round(cm.t["body_inertia"][1], 9))) == 3  # (principal axes = body axes, three different moments)
    for axis in range(3):
        h, _, _k, step, _ = _stepper(be, cm, N, raise_z=1.0, upright=True)
        tau = 0.3
        x = np.zeros((N, 6), f32)
        x[:, 3 + axis] = tau
        s = step(1, x)
        w = s[:, cm.nq + 3:cm.nq + 6]
        np.testing.assert_allclose(w[:, axis], hh * tau / float(cm.t["body_inertia"][1][axis]), rtol=2e-6)
        assert (np.delete(w, axis, 1) == 0).all() and (s[:, cm.nq:cm.nq + 2] == 0).all()
        be.lib.model_close(h)


# ---- 4: env steps against EnvOracle ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_frames", [1, 2])
def test_env_step_xfrc_matches_env_oracle(be, n_frames):
    """tests/test_kernels_physics.py::test_env_step_matches_env_oracle with a wrench on steps 3 .. 8 in four of the seven environments: the kernel re-seeded
    from the oracle state before every step, that test's tolerances."""
    cm = load_model("synth_stompy_pro")
    h, dims, _keep = be.model(cm, True)
    N, O, OP, R, nv, nu = 7, dims.obs_dim, dims.obs_pad, dims.rec_dim, cm.nv, cm.nu
    body = _push_bodies(cm)[1]
    rcfg = RewardCfg(height_min_z=0.95)
    env = EnvOracle(cm.t, rcfg, include_c_vals=True, n_frames=n_frames)
    env.ph = PushedPhysics(cm.t, np.float64, n_frames)
    env.ph.body = body
    state, reset_rec, obs = be.zeros((N, R)), be.zeros((R,)), be.full((N, OP), np.nan)
    rew, done = be.zeros((N,)), be.zeros((N,), np.uint8)
    met = {k: be.full((N,), 7, dt) for k, dt in METRIC_TYPES.items()}
    Ms = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    be.lib.env_reset(h, N, be.ptr(state), be.ptr(reset_rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(Ms), be.stream)
    es = env.reset(N)
    np.testing.assert_allclose(be.host(state), pack(env, es["pipeline_state"], dims, nv), atol=2e-3)
    rc = nat.RewardCfg(rcfg.height_min_z, rcfg.height_max_z, 2.0, 0.2, 0.5, 0.1, 4.0, 1.0, 1.25)
    rng = np.random.default_rng(1)
    pushed_envs = np.array([0, 2, 3, 6])
    n_done, dv_all, dv_pushed, effect = 0, [], [], []
    for t in range(12):
        a = (0.6 * rng.standard_normal((N, nu))).astype(f32)
        x = np.zeros((N, 6), f32)
        if 3 <= t <= 8:
            x[pushed_envs, :3] = rng.uniform(-50, 50, (4, 3))
            x[pushed_envs, 3:] = rng.uniform(-5, 5, (4, 3))
        if t == 5:
            es["pipeline_state"]["qvel"][3, 2] = -30.0  # slammed down: terminates by height
        if t == 9:
            es["pipeline_state"]["qvel"][5, 0] = np.nan  # NaN guard
        be.put(state, pack(env, es["pipeline_state"], dims, nv))
        for k in met:
            be.put(met[k], es["metrics"][k].astype(METRIC_TYPES[k]))
        da, dx = be.arr(a), be.arr(x)
        be.lib.env_step_xfrc(h, N, n_frames, C.byref(rc), be.ptr(state), be.ptr(reset_rec), be.ptr(da), nu, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(Ms),
                             body, be.ptr(dx), be.stream)
        be.sync()
        before = es["pipeline_state"]
        env.ph.xfrc = None
        plain = env.ph.pipeline_step(before, a.astype(f64))
        env.ph.xfrc = x.astype(f64)
        es = env.step(es, a.astype(np.float64))
        s = es["pipeline_state"]
        got_done = be.host(done).astype(bool)
        assert (got_done == es["done"]).all(), (t, got_done, es["done"])
        n_done += int(got_done.sum())
        fin = ~np.isnan(es["reward"])
        np.testing.assert_allclose(be.host(obs)[:, :O], es["obs"], atol=1e-4)
        np.testing.assert_allclose(be.host(rew)[fin], es["reward"][fin], atol=1e-2)
        st = be.host(state)
        np.testing.assert_allclose(st[:, :cm.nq], s.qpos, atol=2e-3 * n_frames)
        ok = ~(got_done | np.isnan(s.qvel).any(1))
        dv_all.append(np.abs(st[:, cm.nq:cm.nq + nv] - s.qvel)[ok].max(1))
        np.testing.assert_allclose(st[:, OP + nv + 1], s.time, atol=1e-6)
        if 3 <= t <= 8:  # the pushed environment-steps on their own: the kernel's distance from the oracle, and how far the wrench moves the oracle itself
            pe = pushed_envs[ok[pushed_envs]]
            dv_pushed.append(np.abs(st[pe, cm.nq:cm.nq + nv] - s.qvel[pe]).max(1))
            effect.append(np.abs(s.qvel[pe] - plain.qvel[pe]).max(1))
        for k in met:
            g, w = be.host(met[k]), es["metrics"][k]
            if METRIC_TYPES[k] == f32:
                np.testing.assert_allclose(g[fin], w[fin], rtol=1e-4, atol=1e-2)
            else:
                assert (g == w).all(), (t, k, g, w)
    assert n_done >= 2
    dv = np.concatenate(dv_all)
    dvp, eff = np.concatenate(dv_pushed), np.concatenate(effect)
    print(f"n_frames {n_frames}: dv max {dv.max():.3e} median {np.median(dv):.3e} share above 0.15 {np.mean(dv > 0.15 * n_frames):.3f}; "
          f"{dvp.size} pushed environment-steps: dv median {np.median(dvp):.3e}, the wrench moves the oracle's qvel by median {np.median(eff):.3e} min {eff.min():.3e}")
    # that test's median bound on the pushed environment-steps alone, where (from the oracle alone) the wrench moves qvel by more than twice that bound in the
    # median: a step that ignored the wrench would sit a wrench's effect away there and miss it
    assert dvp.size >= 16 and np.median(eff) > 2 * 0.02 * n_frames
    assert np.median(dvp) <= 0.02 * n_frames, np.median(dvp)
    assert dv.max() <= 1.0 * n_frames and np.mean(dv > 0.15 * n_frames) <= 0.05 and np.median(dv) <= 0.02 * n_frames, (dv.max(), np.mean(dv > 0.15 * n_frames), np.median(dv))
    be.lib.model_close(h)


# ---- 5: placement changes nothing ---------------------------------------------------------------------------------------------------------------------


def _pushed_steps(be, cm, N=9, steps=6, want_kind=None):
    h, dims, _keep = be.model(cm)
    if want_kind is not None:
        flag = C.c_int32(-1)
        be.lib.model_is_specialized(h, C.byref(flag))
        assert flag.value == want_kind
    OP, R, nu = dims.obs_pad, dims.rec_dim, max(cm.nu, 1)
    state, reset_rec, obs = be.zeros((N, R)), be.zeros((R,)), be.zeros((N, OP))
    rew, done = be.zeros((N,)), be.zeros((N,), np.uint8)
    be.lib.env_reset(h, N, be.ptr(state), be.ptr(reset_rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), None, be.stream)
    rc = nat.RewardCfg(-1.0, 2.0, *RC[2:])
    rng = np.random.default_rng(3)
    body = _push_bodies(cm)[1]
    for _ in range(steps):
        act = be.arr((0.8 * rng.standard_normal((N, nu))).astype(f32))
        x = be.arr(np.concatenate([rng.uniform(-50, 50, (N, 3)), rng.uniform(-5, 5, (N, 3))], 1).astype(f32))
        be.lib.env_step_xfrc(h, N, 2, C.byref(rc), be.ptr(state), be.ptr(reset_rec), be.ptr(act), nu, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), None, body, be.ptr(x),
                             be.stream)
        be.sync()
    out = dict(state=be.host(state).copy(), obs=be.host(obs).copy(), rew=be.host(rew).copy(), done=be.host(done).copy())
    be.lib.model_close(h)
    return out


def test_pushed_steps_are_the_same_bits_under_every_placement(be, monkeypatch):
    """The switches of test_specialised_kernel_equals_the_runtime_sized_kernel and test_matrices_in_global_memory_change_nothing: six pushed steps on the
    library's instantiation, on the run-time-sized kernel and with the matrices in LDS / in global memory."""
    for which in ("pro", "export_biped"):
        cm = _cm(which)
        monkeypatch.delenv("MPPO_ENV_GENERIC", raising=False)
        monkeypatch.delenv("MPPO_ENV_SPILL", raising=False)
        spec = _pushed_steps(be, cm, want_kind=1)
        assert np.isfinite(spec["state"]).all()
        monkeypatch.setenv("MPPO_ENV_GENERIC", "1")
        ph.assert_bit_equal(spec, _pushed_steps(be, cm, want_kind=0))
        monkeypatch.delenv("MPPO_ENV_GENERIC")
        if which == "export_biped":
            for spill in ("0", "1", "3"):
                monkeypatch.setenv("MPPO_ENV_SPILL", spill)
                ph.assert_bit_equal(spec, _pushed_steps(be, cm, want_kind=0))
            monkeypatch.delenv("MPPO_ENV_SPILL")


@pytest.mark.gpu
def test_kernel_compiled_at_start_up_equals_the_runtime_sized_kernel_under_pushes(tmp_path, monkeypatch):
    """environment.jit_kernel's code object for a robot without an instantiation (tests/golden/hand_leg.xml) against the run-time-sized kernel, six pushed steps."""
    import torch  # noqa: F401

    from backends import get_backend
    from minppo_amd import jit

    be = get_backend("hip")
    cm = _cm("hand_leg")
    monkeypatch.setenv(jit.CACHE_ENV, str(tmp_path))
    monkeypatch.delenv("MPPO_TEST_JIT", raising=False)
    image = jit.compile_kernel(jit.dims_of(cm), 48).read_bytes()
    want = _pushed_steps(be, cm, want_kind=0)
    orig = be.model

    def attached(cm_, include_c_vals=True):
        h, dims, keep = orig(cm_, include_c_vals)
        assert jit.attach(be.lib, h, image, 48)
        be.lib.model_get_dims(h, C.byref(dims))
        return h, dims, keep

    monkeypatch.setattr(be, "model", attached)
    ph.assert_bit_equal(want, _pushed_steps(be, cm, want_kind=2))


# ---- 6: the draw inside the kernel equals fill + step ---------------------------------------------------------------------------------------------------

EN, EK, ER, EH = 20, 16, 3, 64
EI, ED = 5, 2
_EVALS = {}


def _eval_setup(be):
    cm = _cm("pro")
    h, dims, keep = be.model(cm)
    net = nat.Net(dims.obs_dim, dims.obs_pad, dims.nu, EH, 1, 0, 2)
    params = init_flat_params(3, dims.obs_dim, dims.nu, EH)
    return cm, h, dims, keep, net, params


def _ecfg(window=(-0.2, 2.0), k=EK):
    rc = reward_cfg(make_config(BASE, [f"reward.height_min_z={window[0]}", f"reward.height_max_z={window[1]}"]))
    return nat.EvalCfg(N=EN, K=k, n_frames=1, deterministic=1, record_envs=ER, reset_noise_scale=0.0, seed=SEED, reward=rc)


def _table(O):
    rng = np.random.default_rng(4)
    return np.stack([0.05 * rng.standard_normal(O), rng.uniform(0.5, 1.5, O)]).astype(f32)


def _evaluate(be, push, table=None, entry="push", window=(-0.2, 2.0)):
    """mppo_evaluate_push (or _obs_norm) -> (result bytes, trajectory); computed once per backend and argument set."""
    key = (be.name, None if push is None else bytes(push), table is not None, entry, window)
    if key in _EVALS:
        return _EVALS[key]
    cm, h, dims, keep, net, params = _eval_setup(be)
    e = _ecfg(window)
    need = be.lib.eval_ws_bytes(h, C.byref(net), C.byref(e))
    ws = be.full((need,), 0xA5, np.uint8)
    res = be.full((C.sizeof(nat.EvalResultRaw) // 8,), -1, np.int64)
    traj = be.full((EK + 1, ER, cm.nq + cm.nv + dims.nu + 2), np.nan)
    p_dev, t_dev = be.arr(params), be.arr(table) if table is not None else None
    if entry == "push":
        be.lib.evaluate_push(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), need, be.ptr(t_dev), 5.0, C.byref(push) if push is not None else None, be.ptr(res),
                             be.ptr(traj), be.stream)
    else:
        be.lib.evaluate_obs_norm(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), need, be.ptr(t_dev), 5.0, be.ptr(res), be.ptr(traj), be.stream)
    be.sync()
    out = (be.host(res).tobytes(), be.host(traj).copy())
    be.lib.model_close(h)
    _EVALS[key] = out
    return out


def _by_hand(be, push, table=None):
    """The documented sequence of mppo_evaluate_push written out with the library's entry points."""
    cm, h, dims, keep, net, params = _eval_setup(be)
    e = _ecfg()
    lib, s = be.lib, be.stream
    OP, RD, A, nqv = dims.obs_pad, dims.rec_dim, dims.nu, cm.nq + cm.nv
    W = nqv + A + 2
    state, rec, obs = be.zeros((EN, RD)), be.zeros((RD,)), be.zeros((EN, OP))
    rew, done = be.zeros((EN,)), be.zeros((EN,), np.uint8)
    met = {k: be.full((EN,), 3, t) for k, t in METRIC_TYPES.items()}
    Ms = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    p_dev, t_dev = be.arr(params), be.arr(table) if table is not None else None
    act, logp, val, noise, xfrc = be.zeros((EN, A)), be.zeros((EN,)), be.zeros((EN,)), be.zeros((EN, A)), be.full((EN, 6), np.nan)
    wsb = lib.policy_ws_bytes(C.byref(net), EN)
    ws = be.zeros((wsb,), np.uint8)
    acc = be.full((nat.EVAL_ACC_SLOTS * EN,), -1, np.int64)
    res = be.full((C.sizeof(nat.EvalResultRaw) // 8,), -1, np.int64)
    traj = be.zeros((EK + 1, ER, W))
    pf = nat.PushCfg.from_buffer_copy(push)
    pf.rank, pf.seed = 0, e.seed
    lib.env_reset(h, EN, be.ptr(state), be.ptr(rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(Ms), s)
    be.sync()
    frame0 = np.zeros((ER, W), f32)
    frame0[:, :nqv] = be.host(state)[:ER, :nqv]
    rows = [frame0]
    for t in range(EK):
        lib.policy_forward(C.byref(net), be.ptr(p_dev), EN, be.ptr(obs), OP, be.ptr(noise), be.ptr(act), be.ptr(logp), be.ptr(val), 0, be.ptr(ws), wsb, s)
        lib.push_fill(C.byref(pf), EN, None, 0, t, be.ptr(xfrc), s)
        lib.env_step_xfrc(h, EN, e.n_frames, C.byref(e.reward), be.ptr(state), be.ptr(rec), be.ptr(act), A, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(Ms),
                          push.body, be.ptr(xfrc), s)
        if table is not None:
            lib.obs_norm_apply(EN, net.O, be.ptr(obs), OP, be.ptr(t_dev), net.O, 5.0, None, s)
        row = be.zeros((ER, W))
        lib.eval_accumulate(EN, int(t == 0), be.ptr(rew), be.ptr(done), C.byref(Ms), be.ptr(acc), be.ptr(state), RD, nqv, be.ptr(act), A, A, ER, be.ptr(row), s)
        be.sync()
        rows.append(be.host(row).copy())
    lib.eval_reduce(EN, EK, be.ptr(acc), be.ptr(res), s)
    be.sync()
    out = (be.host(res).tobytes(), np.stack(rows))
    lib.model_close(h)
    return out


@pytest.mark.parametrize("normed", [False, True])
def test_evaluate_push_is_fill_plus_step(be, normed):
    push = _pcfg(body=_push_bodies(_cm("pro"))[1], interval=EI, duration=ED, rank=3, seed=999)  # (rank and seed of the configuration are not read)
    table = _table(_cm("pro").obs_size(True)) if normed else None
    raw, traj = _evaluate(be, push, table)
    raw_h, traj_h = _by_hand(be, push, table)
    assert not np.isnan(traj).any()
    assert np.array_equal(_bits(traj), _bits(traj_h))
    assert raw == raw_h
    # push = NULL and force = 0: mppo_evaluate_obs_norm
    plain = _evaluate(be, None, table, entry="obs_norm")
    for off in (None, _pcfg(force=0.0, interval=EI, duration=ED)):
        got = _evaluate(be, off, table)
        assert got[0] == plain[0] and np.array_equal(_bits(got[1]), _bits(plain[1]))
    assert not np.array_equal(traj, plain[1])


def test_evaluate_push_refuses_bad_configurations(be):
    cm, h, dims, keep, net, params = _eval_setup(be)
    e = _ecfg(k=2)
    need = be.lib.eval_ws_bytes(h, C.byref(net), C.byref(e))
    ws, res, p_dev = be.zeros((need,), np.uint8), be.zeros((12,), np.int64), be.arr(params)
    traj = be.zeros((3, ER, cm.nq + cm.nv + dims.nu + 2))
    f = be.lib._fn["mppo_evaluate_push"]
    for bad, word in ((_pcfg(body=0), "push body"), (_pcfg(body=cm.nbody), "push body"), (_pcfg(force=-2.0), "negative"), (_pcfg(interval=0), "interval"),
                      (_pcfg(duration=I + 1), "duration")):
        assert f(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), need, 0, 0.0, C.byref(bad), be.ptr(res), be.ptr(traj), be.stream) != 0
        assert word in be.lib.last_error(), (word, be.lib.last_error())
    be.lib.model_close(h)


ENGINE = ["training.num_envs=32", "training.num_steps=3", "rl.num_env_steps=3", "training.num_minibatches=2", "training.update_epochs=1", "model.hidden_size=32",
          "training.total_timesteps=100000"]
PUSHED = [f"environment.push_force={F}", f"environment.push_interval={EI}", f"environment.push_duration={ED}", "environment.push_body=left_shin"]


def test_engine_rollout_is_fill_plus_step(be):
    """Updates 0 and 1 of a pushed engine replayed by hand from the state each started from: the engine's own actions, mppo_push_fill with the update index
    in a device word (mul = T, add = t), mppo_env_step_xfrc - the engine's state, obs, reward and done regions bit for bit."""
    cfg = make_config(BASE, ENGINE + PUSHED)
    tr = be.trainer(cfg)
    cm, N, T, OP, A = tr.cm, tr.N, tr.T, tr.OP, tr.A
    R = int(tr.dims.rec_dim)
    body = list(cm.body_names).index("left_shin")
    assert tr.push.body == body
    tr.reset()
    tr._sync()
    h, dims, _keep = be.model(cm)
    pf = _pcfg(body=body, interval=EI, duration=ED, rank=0, seed=tr.seed)
    any_push = 0
    for u in range(2):
        start = tr._to_host(tr.region("state", (N, R))).copy()
        tr.update()
        tr._sync()
        eng = {k: tr._to_host(tr.region(k, shp)).copy() for k, shp in (("state", (N, R)), ("obs", (T + 1, N, OP)), ("reward", (T, N)), ("done", (T, N)), ("action", (T, N, A)))}
        assert int(tr._to_host(tr.region("count"))[1]) == u + 1
        state, reset_rec = be.arr(start), be.arr(tr._to_host(tr.region("reset_rec")).copy())
        ctr = be.arr(np.array([u], np.int32))
        obs, rew, done, xfrc = be.zeros((N, OP)), be.zeros((N,)), be.zeros((N,), np.uint8), be.zeros((N, 6))
        for t in range(T):
            act = be.arr(eng["action"][t])
            be.lib.push_fill(C.byref(pf), N, be.ptr(ctr), T, t, be.ptr(xfrc), be.stream)
            be.lib.env_step_xfrc(h, N, 1, C.byref(tr.ecfg.reward), be.ptr(state), be.ptr(reset_rec), be.ptr(act), A, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), None, body,
                                 be.ptr(xfrc), be.stream)
            be.sync()
            want = jaxrng.push_wrench_philox(tr.seed, 0, u * T + t, N, F, EI, ED)
            assert np.array_equal(_bits(be.host(xfrc)), _bits(want))
            any_push += int((want != 0).any(1).sum())
            assert np.array_equal(_bits(be.host(obs)), _bits(eng["obs"][t + 1])), (u, t)
            assert np.array_equal(_bits(be.host(rew)), _bits(eng["reward"][t])) and np.array_equal(be.host(done), eng["done"][t]), (u, t)
        assert np.array_equal(_bits(be.host(state)), _bits(eng["state"])), u
    assert any_push >= N  # (interval 5, duration 2, six steps: every environment is pushed at least once)
    be.lib.model_close(h)
    tr.close()


# ---- 7: where a pushed evaluation leaves the unpushed one ---------------------------------------------------------------------------------------------


def test_trajectories_part_at_the_first_pushed_step(be):
    push = _pcfg(body=1, interval=EI, duration=ED)
    _, plain = _evaluate(be, None, None, entry="obs_norm")
    _, pushed = _evaluate(be, push, None)
    w = np.stack([jaxrng.push_wrench_philox(SEED, 0, s, EN, F, EI, ED) for s in range(EK)])
    assert not plain[..., -1].any() and not pushed[..., -1].any()  # nobody fell: no restart hides a difference
    firsts = []
    for n in range(ER):
        first = int(np.argmax((w[:, n] != 0).any(1)))
        assert (w[first, n] != 0).any()
        firsts.append(first)
        assert np.array_equal(_bits(plain[:first + 1, n]), _bits(pushed[:first + 1, n])), n  # frames 0 .. first: the states before the first pushed step
        assert not np.array_equal(plain[first + 1, n], pushed[first + 1, n]), n
    assert len(set(firsts)) > 1  # the recorded environments are not all in phase


# ---- 8: the engine's surface ----------------------------------------------------------------------------------------------------------------------------


def _arena(tr, names=("params", "adam_m", "adam_v", "count", "state", "episode_returns", "episode_lengths", "returned_episode")):
    tr._sync()
    return {n: tr._to_host(tr.region(n)).copy() for n in names}


def _run(be, cfg, updates, before=None, **kw):
    tr = be.trainer(cfg, **kw)
    if before is not None:
        before(tr)
    tr.reset()
    for _ in range(updates):
        tr.update()
    out = _arena(tr)
    graph = tr.graph_active()
    tr.close()
    return out, graph


def test_force_zero_is_an_engine_that_never_heard_of_pushes(be):
    cfg = make_config(BASE, ENGINE)
    never, _ = _run(be, cfg, 2)
    off = nat.PushCfg(body=0, interval=0, duration=0, rank=0, force=0.0, seed=0)  # (force 0: nothing else is read - not even the body)
    zero, _ = _run(be, cfg, 2, before=lambda tr: be.lib.engine_set_push(tr._engine, C.byref(off)))
    null, _ = _run(be, cfg, 2, before=lambda tr: be.lib.engine_set_push(tr._engine, None))
    pushed, _ = _run(be, make_config(BASE, ENGINE + PUSHED), 2)
    for k in never:
        assert np.array_equal(_bits(never[k]), _bits(zero[k])) and np.array_equal(_bits(never[k]), _bits(null[k])), k
    assert not np.array_equal(never["state"], pushed["state"]) and np.isfinite(pushed["params"]).all()


def test_pushed_engine_checkpoints_and_resumes(be, tmp_path):
    cfg = make_config(BASE, ENGINE + PUSHED)
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
    assert tr.graph_active() == (be.name == "hip")
    tr.close()
    c = be.trainer(cfg)
    c.load_checkpoint(ck)
    for _ in range(2):
        c.update()
    c4 = _arena(c)
    c.close()
    for k in a4:
        assert np.array_equal(_bits(a4[k]), _bits(c4[k])), k
    if be.name == "hip":  # a replayed graph draws what eager launches draw
        e3, graph = _run(be, cfg, 3, use_graph=False)
        assert not graph
        for k in a3:
            assert np.array_equal(_bits(a3[k]), _bits(e3[k])), k


def test_set_push_call_order_and_refusals(be):
    tr = be.trainer(make_config(BASE, ENGINE))
    f = be.lib._fn["mppo_engine_set_push"]
    nb = tr.cm.nbody
    for bad, word in ((_pcfg(body=0), "push body"), (_pcfg(body=nb), "push body"), (_pcfg(force=-1.0), "negative"), (_pcfg(force=float("nan")), "negative"),
                      (_pcfg(interval=0), "interval"), (_pcfg(duration=0), "duration"), (_pcfg(duration=I + 1), "duration")):
        assert f(tr._engine, C.byref(bad)) != 0 and word in be.lib.last_error(), word
    be.lib.engine_set_push(tr._engine, C.byref(_pcfg()))
    be.lib.engine_set_push(tr._engine, None)
    tr.reset()
    assert f(tr._engine, C.byref(_pcfg())) == -4 and "mppo_engine_reset has run" in be.lib.last_error()  # MPPO_ESTATE
    tr.lib.engine_prepare(tr._engine, tr._stream_ptr)
    tr._sync()
    assert f(tr._engine, C.byref(_pcfg())) == -4
    assert "mppo_engine_set_push" in be.lib.last_error() and "prepared" in be.lib.last_error()
    with pytest.raises(nat.NativeError):
        be.lib.engine_set_push(tr._engine, C.byref(_pcfg()))
    tr.close()


# ---- 9: the host surface ------------------------------------------------------------------------------------------------------------------------------


def test_config_keys_defaults_and_refusals():
    env = make_config(BASE).environment
    assert (env.push_force, env.push_interval, env.push_duration, env.push_body) == (0.0, 1000, 50, "")
    got = make_config(BASE, ["environment.push_force=25", "environment.push_interval=200", "environment.push_duration=10", "environment.push_body=torso"]).environment
    assert (got.push_force, got.push_interval, got.push_duration, got.push_body) == (25.0, 200, 10, "torso")
    with pytest.raises(ValueError, match="push_force"):
        make_config(BASE, ["environment.push_force=-1"])
    for bad in (["environment.push_interval=0"], ["environment.push_duration=0"], ["environment.push_interval=10", "environment.push_duration=11"]):
        with pytest.raises(ValueError, match="push_interval"):
            make_config(BASE, ["environment.push_force=5"] + bad)
        make_config(BASE, bad)  # (read only when push_force > 0)


def test_unknown_push_body_names_the_bodies():
    from minppo_amd.train import push_body_id, push_cfg, resolve_model

    with pytest.raises(ValueError, match=r"push_body.*nose.*torso.*left_shin"):
        resolve_model(make_config(BASE, ["environment.push_force=5", "environment.push_body=nose"]))
    with pytest.raises(ValueError, match="push_body"):
        resolve_model(make_config(BASE, ["environment.push_force=5", "environment.push_body=world"]))
    cm = resolve_model(make_config(BASE, ["environment.push_body=nose"]))  # (pushes off: the name is not read)
    assert push_cfg(make_config(BASE), cm) is None
    p = push_cfg(make_config(BASE, ["environment.push_force=5", "environment.push_body=left_shin"]), cm, seed=9, rank=2)
    assert (p.body, p.interval, p.duration, p.rank, p.force, p.seed) == (list(cm.body_names).index("left_shin"), 1000, 50, 2, 5.0, 9)
    assert push_cfg(make_config(BASE, ["environment.push_force=5"]), cm).body == 1
    # HumanoidEnv resolves the name whatever the force is: step(..., xfrc=) is an explicit wrench and needs no random draw
    named = make_config(BASE, ["environment.push_body=left_shin"])
    assert push_body_id(named, cm) == 1 and push_body_id(named, cm, always=True) == list(cm.body_names).index("left_shin")
    with pytest.raises(ValueError, match=r"push_body.*nose.*left_shin"):
        push_body_id(make_config(BASE, ["environment.push_body=nose"]), cm, always=True)


def test_python_evaluate_goes_through_the_pushed_entry_point(be):
    from minppo_amd.evaluate import evaluate, result_from_struct

    push = _pcfg(body=1, interval=EI, duration=ED)
    raw, traj = _evaluate(be, push, None)
    cfg = make_config(BASE, [f"model.hidden_size={EH}", f"training.seed={SEED}", f"evaluation.num_envs={EN}", f"evaluation.num_steps={EK}", f"evaluation.record_envs={ER}",
                             f"environment.push_force={F}", f"environment.push_interval={EI}", f"environment.push_duration={ED}"])
    cm = _cm("pro")
    flat = init_flat_params(3, cm.obs_size(True), cm.nu, EH)
    device = {} if be.name == "emu" else {"device": "cuda:0"}
    got = evaluate(cfg, flat, lib=be.lib, xp=be.xp, **device)
    assert got.stats() == result_from_struct(nat.EvalResultRaw.from_buffer_copy(raw)).stats()
    assert set(got.trajectory) == {"qpos", "qvel", "action", "reward", "done"}
    assert np.array_equal(_bits(got.trajectory["qpos"]), _bits(traj[..., :cm.nq]))


@pytest.mark.gpu
def test_humanoid_env_takes_a_wrench_and_draws_the_pushes():
    import torch

    from minppo_amd.env import HumanoidEnv

    over = [f"environment.push_force={F}", f"environment.push_interval={I}", f"environment.push_duration={D}", "environment.push_body=left_shin", f"training.seed={SEED}"]
    env = HumanoidEnv(make_config(BASE, over))
    N = 5
    cm = env.cm
    body = list(cm.body_names).index("left_shin")
    for s in (0, 4):
        assert np.array_equal(_bits(env.push_wrench(s, N).cpu().numpy()), _bits(jaxrng.push_wrench_philox(SEED, 0, s, N, F, I, D)))
    assert np.array_equal(_bits(env.push_wrench(2, N, seed=77).cpu().numpy()), _bits(jaxrng.push_wrench_philox(77, 0, 2, N, F, I, D)))
    es = env.reset(num_envs=N)
    act = 0.3 * torch.ones(N, env.action_size, device=env.device)
    x = torch.from_numpy(np.concatenate([np.random.default_rng(2).uniform(-50, 50, (N, 3)), np.zeros((N, 3))], 1).astype(f32))
    e1 = env.step(es, act, xfrc=x)
    # the C call
    lib, d = env.lib, env.dims
    state = es.pipeline_state.clone()
    obs = torch.empty(N, d.obs_pad, device=env.device)
    rew, done, xd = torch.empty(N, device=env.device), torch.empty(N, dtype=torch.uint8, device=env.device), x.to(env.device)
    lib.env_step_xfrc(env._model, N, 1, C.byref(env._rc), state.data_ptr(), env._reset_rec.data_ptr(), act.data_ptr(), env.action_size, obs.data_ptr(), d.obs_pad,
                      rew.data_ptr(), done.data_ptr(), None, body, xd.data_ptr(), torch.cuda.current_stream(env.device).cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(e1.pipeline_state, state) and torch.equal(e1.reward, rew)
    e0 = env.step(es, act)
    assert not torch.equal(e0.pipeline_state, e1.pipeline_state)
    assert torch.equal(env.step(es, act, xfrc=torch.zeros(N, 6)).pipeline_state, e0.pipeline_state)
    for bad in (torch.zeros(N, 3), torch.zeros(N + 1, 6), torch.zeros(6)):
        with pytest.raises(ValueError, match="xfrc"):
            env.step(es, act, xfrc=bad)
    env.close()
    plain = HumanoidEnv(make_config(BASE))
    with pytest.raises(ValueError, match="push_force"):
        plain.push_wrench(0, N)
    plain.close()
    # an explicit wrench needs no random draw: at push_force = 0 it still acts on the named body, and an unknown name is refused when the model is opened
    named = HumanoidEnv(make_config(BASE, ["environment.push_body=left_shin"]))
    assert named._push_body == body and named._push is None
    e2 = named.step(named.reset(num_envs=N), act, xfrc=x)
    assert torch.equal(e2.pipeline_state, e1.pipeline_state)
    named.close()
    with pytest.raises(ValueError, match=r"push_body.*nose.*left_shin"):
        HumanoidEnv(make_config(BASE, ["environment.push_body=nose"]))


@pytest.mark.gpu
def test_train_and_evaluate_under_pushes_from_the_command_line(tmp_path):
    model = str(tmp_path / "model.pkl")
    small = ["training.num_envs=64", "training.num_minibatches=2", "model.hidden_size=64", f"environment.push_force={F}", f"environment.push_interval={EI}",
             f"environment.push_duration={ED}", "environment.push_body=torso"]
    p = subprocess.run([sys.executable, "-m", "minppo_amd.cli", "train", "stompy_pro", *small, "training.total_timesteps=1280", f"training.model_save_path={model}"],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert p.returncode == 0 and Path(model).exists(), p.stderr[-2000:]
    p = subprocess.run([sys.executable, "-m", "minppo_amd.cli", "evaluate", "stompy_pro", *small, "evaluation.num_envs=20", "evaluation.num_steps=8",
                        f"inference.model_path={model}"], capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1
    assert set(json.loads(line[0])) == {"episodes", "mean_return", "std_return", "min_return", "max_return", "mean_length", "min_length", "max_length", "survivors",
                                         "survivor_mean_return", "mean_reward", "steps"}
    assert json.loads(line[0])["steps"] == 160
