"""What the physics tests share (a plain module, imported by name): the kernel's forward probe, the float64 / float32 pair of the oracle with
the "well-conditioned poses" filter, THE definition of "the kernel follows the oracle" (check_against_oracle), bit-equality across kernel
instantiations and placements, the start-up-compiled kernel and reproducible training on a fixture, the state and model generators several
test modules use, and the oracle's recording on the committed models (tests/golden/oracle_features.npz)."""

import ctypes as C
from pathlib import Path

import numpy as np

from minppo_amd import _native as nat
from minppo_amd import mjcf
from minppo_amd.model import BUILTIN_MODELS, JNT_BALL, JNT_FREE, compile_model, load_model
from oracle.physics_oracle import Physics, PhysState, qmul
from oracle.physics_oracle import integrate_positions as _integrate_positions

f32, f64 = np.float32, np.float64
GOLDEN = Path(__file__).parent / "golden"
SMOOTH_TOL = dict(qM=2e-5, qfrc_bias=2e-4, qacc_smooth=5e-4, xpos=1e-5)  # float32 kernel against float64 oracle, of each quantity's largest magnitude


# ---------------------------------------------------------------------------------------------------------------------------------------
# the kernel's side
# ---------------------------------------------------------------------------------------------------------------------------------------


def probe(be, h, cm, qpos, qvel, ctrl, warm):
    """mppo_physics_forward on N states: every intermediate quantity of one forward pass, as host arrays."""
    N = qpos.shape[0]
    nv, nb, nefc = cm.nv, cm.nbody, max(cm.nefc, 1)
    shapes = dict(qM=(N, nv, nv), qfrc_bias=(N, nv), qfrc_passive=(N, nv), qfrc_actuator=(N, nv), qacc_smooth=(N, nv), efc_J=(N, nefc, nv),
                  efc_D=(N, nefc), efc_aref=(N, nefc), qacc=(N, nv), cinert=(N, nb, 10), cvel=(N, nb, 6), subtree_com1=(N,), xpos=(N, nb, 3),
                  qacc_euler=(N, nv))
    out = {k: be.zeros(s) for k, s in shapes.items()}
    niter = be.zeros((N,), np.int32)
    d_in = [be.arr(x.astype(f32)) for x in (qpos, qvel, ctrl if cm.nu else np.zeros((N, 1)), warm)]
    pr = nat.ForwardProbe(**{k: be.ptr(v) for k, v in out.items()}, solver_niter=be.ptr(niter))
    be.lib.physics_forward(h, N, be.ptr(d_in[0]), be.ptr(d_in[1]), be.ptr(d_in[2]) if cm.nu else 0, be.ptr(d_in[3]), C.byref(pr), be.stream)
    res = {k: be.host(v) for k, v in out.items()}
    res["niter"] = be.host(niter)
    return res


def cost(ref, qacc):
    """The Gauss cost of `qacc` on the oracle's rows (inequality rows: active where J qacc - aref < 0)."""
    qacc = qacc.astype(np.float64)
    jar = np.einsum("nrv,nv->nr", ref.efc_J, qacc) - ref.efc_aref
    Ma = np.einsum("nij,nj->ni", ref.qM, qacc)
    return 0.5 * np.sum(ref.efc_D * jar * jar * (jar < 0), -1) + 0.5 * np.sum((Ma - ref.qfrc_smooth) * (qacc - ref.qacc_smooth), -1)


def euler_acc(cm, ref):
    """the acceleration the integrator applies (MJX euler with implicit joint damping):
    (M + h diag(damping))^-1 (qfrc_smooth + qfrc_constraint) - for an undamped model too (MJX has no test for that; physics_oracle.euler)"""
    damp = np.asarray(cm.t["dof_damping"], np.float64)
    dh = ref.qM + float(cm.t["timestep"]) * np.eye(cm.nv)[None] * damp[None, :, None]
    return np.linalg.solve(dh, (ref.qfrc_smooth + ref.qfrc_constraint)[..., None])[..., 0]


def pack(env, s, dims, nv):
    """The kernel's state record of the oracle state `s`."""
    N = s.qpos.shape[0]
    O, OP = dims.obs_dim, dims.obs_pad
    rec = np.zeros((N, dims.rec_dim), f32)
    rec[:, :O] = env.get_obs(s)
    rec[:, OP:OP + nv] = s.qacc_warmstart
    rec[:, OP + nv] = s.subtree_com[:, 1, 0]
    rec[:, OP + nv + 1] = s.time
    return rec


def step_once(be, h, N=4):
    """A reset and one env step of an opened model (the blob fuzzers: an accepted blob must step without a fault)."""
    dims = nat.ModelDims()
    be.lib.model_get_dims(h, C.byref(dims))
    OP, R = dims.obs_pad, dims.rec_dim
    state, reset_rec, obs = be.zeros((N, R)), be.zeros((R,)), be.zeros((N, OP))
    rew, done = be.zeros((N,)), be.zeros((N,), np.uint8)
    be.lib.env_reset(h, N, be.ptr(state), be.ptr(reset_rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), None, be.stream)
    rc = nat.RewardCfg(-0.2, 2.0, 2.0, 0.2, 0.5, 0.1, 4.0, 1.0, 1.25)
    a = be.zeros((N, max(dims.nu, 1)))
    be.lib.env_step(h, N, 1, C.byref(rc), be.ptr(state), be.ptr(reset_rec), be.ptr(a), max(dims.nu, 1), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), None, be.stream)


def run_steps(lib, h, dims, N, steps, torch, seed=0, start=None, actions=None):
    """`steps` env steps of the HIP library on cuda tensors under random actions -> [(state, observation, reward, done)] per step.
    `start`, `actions`: lists that receive the records after the reset and every step's actions (host arrays)."""
    state = torch.zeros(N, dims.rec_dim, device="cuda")
    reset = torch.zeros(dims.rec_dim, device="cuda")
    obs = torch.zeros(N, dims.obs_pad, device="cuda")
    rew = torch.zeros(N, device="cuda")
    done = torch.zeros(N, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    lib.env_reset(h, N, state.data_ptr(), reset.data_ptr(), obs.data_ptr(), dims.obs_pad, 0, 0, None, s)
    if start is not None:
        torch.cuda.synchronize()
        start.append(state.cpu().numpy().copy())
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    rc = nat.RewardCfg(-0.2, 2.0, 2.0, 0.2, 0.5, 0.1, 4.0, 1.0, 1.25)
    out = []
    nu = max(dims.nu, 1)
    for _ in range(steps):
        act = torch.randn(N, nu, device="cuda", generator=g)
        lib.env_step(h, N, 1, C.byref(rc), state.data_ptr(), reset.data_ptr(), act.data_ptr(), nu, obs.data_ptr(), dims.obs_pad, rew.data_ptr(), done.data_ptr(), None, s)
        torch.cuda.synchronize()
        if actions is not None:
            actions.append(act.cpu().numpy().copy())
        out.append((state.cpu().numpy().copy(), obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), done.cpu().numpy().copy()))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# models and states
# ---------------------------------------------------------------------------------------------------------------------------------------


def existing_models():
    """Every built-in robot and every fixture that predates per-row contact parameters: (name, maker).  tests/golden/table_sha256.json pins their tables."""
    out = [(n, lambda f=f: compile_model(f())) for n, f in sorted(BUILTIN_MODELS.items())]
    for p in sorted(list(GOLDEN.glob("*.xml")) + [GOLDEN / "export_biped" / "robot.xml"]):
        if p.name != "contact_params_humanoid.xml":
            out.append((str(p.relative_to(GOLDEN)), lambda p=p: compile_model(mjcf.load_mjcf(str(p)))))
    return out


def many_dof_robot():
    """The 26-dof stand-in with a 4-joint neck and two 5-joint tails: 40 dofs, 37 bodies - past what the model-specialised kernels and the
    register Cholesky cover (32 dofs), so the run-time-sized kernel's LDS factorisation (two triangular work copies) is what runs."""
    from minppo_amd import model as M

    spec = M.synth_stompy_full()
    extra, acts = [], []

    def chain(prefix, parent, n, pos0, axis_cycle, step):
        par = parent
        for k in range(n):
            name = f"{prefix}{k}"
            extra.append(M.BodySpec(name, par, pos=pos0 if k == 0 else step, mass=0.3, inertia=(0.0008, 0.0008, 0.0004), ipos=(0.0, 0.0, 0.5 * step[2]),
                                    joints=[M.JointSpec(name, M.JNT_HINGE, axis=axis_cycle[k % len(axis_cycle)], range=(-0.7, 0.7), damping=0.5, armature=0.02)],
                                    geoms=[M.GeomSpec(M.GEOM_SPHERE, (0.03,), pos=(0.0, 0.0, step[2]))] if k == n - 1 else []))
            acts.append(M.ActuatorSpec(name, kp=8.0, kv=0.0, ctrlrange=(-1.0, 1.0), forcerange=(-10.0, 10.0)))
            par = name

    chain("neck", "torso", 4, (0.0, 0.0, 0.40), [(0, 1, 0), (1, 0, 0), (0, 0, 1)], (0.0, 0.0, 0.06))
    chain("tail_l", "torso", 5, (-0.10, 0.05, 0.0), [(0, 1, 0), (1, 0, 0)], (0.0, 0.0, -0.09))
    chain("tail_r", "torso", 5, (-0.10, -0.05, 0.0), [(0, 1, 0), (1, 0, 0)], (0.0, 0.0, -0.09))
    return M.compile_model(M.ModelSpec(name="many_dof", bodies=spec.bodies + extra, actuators=spec.actuators + acts, free_root_z=spec.free_root_z))


def random_states(cm, N, rng):
    """Random poses of a random robot (tests/test_model_fuzz.py): free bodies turned at random, limited joints inside their range or a little
    beyond it, the first tree set down on the ground -> qpos, qvel, ctrl."""
    t = cm.t
    q = np.tile(np.asarray(t["qpos0"], f64), (N, 1))
    for j in range(cm.njnt):
        qa = int(t["jnt_qposadr"][j])
        if int(t["jnt_type"][j]) == JNT_FREE:
            q[:, qa:qa + 2] += 0.05 * rng.normal(size=(N, 2))
            q[:, qa + 2] += rng.uniform(-0.1, 0.1, N)
            x = rng.normal(size=(N, 4))
            q[:, qa + 3:qa + 7] = x / np.linalg.norm(x, axis=1, keepdims=True)
        elif int(t["jnt_limited"][j]):
            # inside the range, a third of the time 5 - 30 mrad beyond one end of it (limit rows fire, by an amount a joint really reaches:
            # a limit violated by a radian is to six CG iterations what a 30 cm overlap is - see test_twin_follows_the_oracle_on_a_random_robot)
            lo, hi = (float(x) for x in t["jnt_range"][j])
            inside = rng.uniform(lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo), N)
            beyond = np.where(rng.random(N) < 0.5, lo - rng.uniform(0.005, 0.03, N), hi + rng.uniform(0.005, 0.03, N))
            q[:, qa] = np.where(rng.random(N) < 0.33, beyond, inside)
        else:
            q[:, qa] += rng.uniform(-1.4, 1.4, N)
    # the first tree set down so that its lowest collider is between 1 cm inside the ground and 2 cm above it
    if cm.ncon > cm.npair:
        ph = Physics(t)
        d = ph.make_data(N)
        d["qpos"] = q.copy()
        ph.kinematics(d); ph.com_pos(d); ph.collision(d)
        ground = d["con_dist"][:, :cm.ncon - cm.npair]
        mine = np.asarray(t["body_rootid"])[np.asarray(t["con_bodyid"])[:cm.ncon - cm.npair]] == 1
        if mine.any():
            low = np.where(mine[None] & (ground < 0.99), ground, np.inf).min(1)   # (an unused hull slot reads 1)
            q[:, 2] += np.where(np.isfinite(low), rng.uniform(-0.01, 0.02, N) - low, 0.0)
    return q, 0.5 * rng.normal(size=(N, cm.nv)), rng.uniform(-1.3, 1.3, size=(N, cm.nu))


def rot_quat(v):
    """Unit quaternions of rotation vectors [..., 3]."""
    v = np.asarray(v, f64)
    a = np.linalg.norm(v, axis=-1, keepdims=True)
    u = v / np.where(a > 0, a, 1.0)
    return np.concatenate([np.cos(a / 2), u * np.sin(a / 2)], -1)


def start_states(cm, N, rng, spread=0.05):
    """qpos0 with every scalar joint moved by noise and every ball quaternion turned by a small random rotation."""
    q = np.tile(np.asarray(cm.t["qpos0"], f64), (N, 1))
    for j in range(cm.njnt):
        qa, jt = int(cm.t["jnt_qposadr"][j]), int(cm.t["jnt_type"][j])
        if jt == JNT_BALL:
            q[:, qa:qa + 4] = qmul(q[:, qa:qa + 4], rot_quat(spread * rng.standard_normal((N, 3))))
        elif jt != JNT_FREE:
            q[:, qa] += spread * rng.standard_normal(N)
    return q


def walking_states(cm, N, seed, steps=6):
    """States the float64 oracle reaches from near qpos0 under random controls (equalities near satisfied, contacts and limits as they come)
    -> qpos, qvel, ctrl, warm start."""
    ph = Physics(cm.t)
    rng = np.random.default_rng(seed)
    d = ph.pipeline_init(start_states(cm, N, rng), 0.2 * rng.standard_normal((N, cm.nv)))
    for _ in range(steps):
        d = ph.pipeline_step(d, 0.5 * rng.standard_normal((N, cm.nu)))
    return d.qpos, d.qvel, 0.5 * rng.standard_normal((N, cm.nu)), d.qacc_warmstart


# ---------------------------------------------------------------------------------------------------------------------------------------
# the kernel follows the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------


def oracle_pair(cm, q32):
    """One forward pass of the oracle in float64 and in float32 from the float32 states `q32` (qpos, qvel, ctrl, warm start), the
    "well-conditioned" environments - those where the two runs of the ORACLE agree: efc_J within 2e-4 and efc_aref within 5e-4 of their
    scale, equal active sets (a pair normal between nearly coincident points, a row on the edge of switching on, is not) - and
    scale(k) = max |ref[k]| + 1e-6.  -> ref, ref32, good [N], scale"""
    N = q32[0].shape[0]

    def run(dtype):
        d = PhysState(qpos=q32[0].astype(dtype), qvel=q32[1].astype(dtype), ctrl=q32[2].astype(dtype)[:, :cm.nu], qacc_warmstart=q32[3].astype(dtype), time=np.zeros(N, dtype))
        Physics(cm.t, dtype).forward(d)
        return d

    ref, ref32 = run(f64), run(f32)
    scale = lambda k: np.abs(ref[k]).max() + 1e-6
    if ref.efc_D.shape[1] == 0:
        return ref, ref32, np.ones(N, bool), scale
    good = (np.abs(ref32.efc_J - ref.efc_J).reshape(N, -1).max(1) <= 2e-4 * scale("efc_J")) & (np.abs(ref32.efc_aref - ref.efc_aref).max(1) <= 5e-4 * scale("efc_aref")) & \
           ((ref32.efc_D > 0) == (ref.efc_D > 0)).all(1)
    return ref, ref32, good, scale


def check_against_oracle(be, cm, states, what, tol_smooth, tol_rows, min_good, strict_cost):
    """The kernel's forward pass on `states` (qpos, qvel, ctrl, warm start) against the float64 oracle.
      * at least `min_good` well-conditioned environments (oracle_pair) - asserted from the oracle alone, before the kernel is looked at
      * `tol_smooth`: quantities before the constraint, every environment, relative to each quantity's scale
      * the active set, then `tol_rows` (efc_J / efc_D / efc_aref), on the well-conditioned environments; equality rows are always active and
        agree on their own scale too
      * the solver through the Gauss cost it reaches (equality rows active on both signs), where the float32 ORACLE reaches float64's within
        5e-2: within 5e-2 (strict_cost) or, for random robots - stiff, unconverged after six iterations, float32 kernel and float32 oracle
        part by up to 10 % on single poses - 5e-2 in the median and 0.3 at most; never above the unconstrained start; at most six iterations.
        strict_cost None leaves the solver out.
    -> ref, got, good"""
    qpos, qvel, ctrl, warm = states
    N, neq = qpos.shape[0], cm.neq
    q32 = [x.astype(f32) for x in (qpos, qvel, ctrl if cm.nu else np.zeros((N, 1)), warm)]
    ref, ref32, good, scale = oracle_pair(cm, q32)
    assert good.sum() >= min_good, (what, good)
    h, dims, _keep = be.model(cm)
    assert dims.lds_bytes <= 160 * 1024
    got = probe(be, h, cm, *q32)
    be.lib.model_close(h)
    for k, tol in tol_smooth.items():
        r = ref[k]
        if r.size:
            err = np.abs(got[k].reshape(r.shape) - r).max() / scale(k)
            assert err <= tol, (what, k, err)
    if cm.nefc:
        gD = got["efc_D"].reshape(N, -1)
        assert ((gD > 0) == (ref.efc_D > 0))[good].all(), what
        assert (ref.efc_D[:, :neq] > 0).all() and (gD[:, :neq] > 0).all(), what
        for k, tol in tol_rows.items():
            r, g = ref[k], got[k].reshape(ref[k].shape)
            err = np.abs(g[good] - r[good]).max() / scale(k)
            assert err <= tol, (what, k, err)
            if neq:  # the equality rows on their own scale (they come first: efc rows 0 .. neq - 1)
                err = np.abs(g[good, :neq] - r[good, :neq]).max() / (np.abs(r[:, :neq]).max() + 1e-6)
                assert err <= tol, (what, k, "equality rows", err)
    if strict_cost is None:
        return ref, got, good

    def cost_eq(qacc):
        jar = np.einsum("nrv,nv->nr", ref.efc_J[:, :neq], qacc.astype(f64)) - ref.efc_aref[:, :neq]
        return cost(ref, qacc) + 0.5 * np.sum(ref.efc_D[:, :neq] * jar * jar * (jar >= 0), -1)

    c_ref, c32, c_got, c_smooth = cost_eq(ref.qacc), cost_eq(ref32.qacc), cost_eq(got["qacc"]), cost_eq(ref.qacc_smooth)
    conv = good & (np.abs(c32 - c_ref) <= 5e-2 * np.abs(c_ref) + 1e-3)
    rel = np.abs(c_got - c_ref)[conv] / (np.abs(c_ref)[conv] + 1e-3)
    if strict_cost:
        assert rel.max() <= 5e-2, (what, rel)
    else:
        assert np.median(rel) <= 5e-2 and rel.max() <= 0.3, (what, rel)
    assert np.all(c_got <= c_smooth * (1 + 1e-5) + 1e-6), (what, (c_got / c_smooth).max())
    assert np.all(got["niter"] <= 6), (what, got["niter"].max())
    return ref, got, good


# ---------------------------------------------------------------------------------------------------------------------------------------
# after the solver: the integrator, the frames loop and the epilogue from the record's own values (tests/test_step_exact.py)
# ---------------------------------------------------------------------------------------------------------------------------------------

ULP32 = 2.0 ** -24  # one float32 rounding of a unit-scale value
METRIC_TYPES = dict(episode_returns=f32, episode_lengths=np.int32, returned_episode_returns=f32, returned_episode_lengths=np.int32, timestep=np.int32,
                    returned_episode=np.uint8)


def integrate_positions(cm, qpos, qvel_new, h, dtype):
    """The position half of Physics.euler (which calls the same function) on given arrays, in `dtype` arithmetic."""
    return _integrate_positions(cm.t, qpos, qvel_new, h, dtype)


def record_of(dims, cm, qpos, qvel, warm, com_x, time):
    """The kernel's state record from given values (the inverse of `pack`, without an EnvOracle): [qpos, qvel, c-vals and qfrc_actuator zero
    (a step reads them only to copy them out as the observation) | padding | warm start, com_x, time | padding]."""
    N = qpos.shape[0]
    OP, nq, nv = dims.obs_pad, cm.nq, cm.nv
    rec = np.zeros((N, dims.rec_dim), f32)
    rec[:, :nq] = qpos
    rec[:, nq:nq + nv] = qvel
    rec[:, OP:OP + nv] = warm
    rec[:, OP + nv] = com_x
    rec[:, OP + nv + 1] = time
    return rec


class KernelStepper:
    """mppo_env_step of a backend (emulator or HIP library) on host state records."""

    def __init__(self, be, cm):
        self.be, self.cm, self.name = be, cm, be.name
        self.h, self.dims, self._keep = be.model(cm)
        self.reset_rec = self._reset(1)[1]

    def _reset(self, N):
        be, d = self.be, self.dims
        state, reset_rec, obs = be.zeros((N, d.rec_dim)), be.zeros((d.rec_dim,)), be.zeros((N, d.obs_pad))
        be.lib.env_reset(self.h, N, be.ptr(state), be.ptr(reset_rec), be.ptr(obs), d.obs_pad, 0, 0, None, be.stream)
        return be.host(state).copy(), be.host(reset_rec).copy()

    def step(self, rec, action, n_frames, rc, metrics=None):
        """-> record', observation, reward, done (host arrays; `metrics`, a dict of host arrays, is advanced in place)"""
        be, d, N = self.be, self.dims, rec.shape[0]
        nu = max(d.nu, 1)
        state, reset_rec, obs = be.arr(rec.astype(f32)), be.arr(self.reset_rec), be.full((N, d.obs_pad), np.nan)
        rew, done = be.zeros((N,)), be.zeros((N,), np.uint8)
        act = be.arr(np.zeros((N, nu), f32) if d.nu == 0 else action.astype(f32))
        met = {k: be.arr(np.asarray(metrics[k], METRIC_TYPES[k])) for k in METRIC_TYPES} if metrics is not None else None
        M = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()}) if met else None
        be.lib.env_step(self.h, N, n_frames, C.byref(nat.RewardCfg(*rc)), be.ptr(state), be.ptr(reset_rec), be.ptr(act), nu, be.ptr(obs), d.obs_pad, be.ptr(rew),
                        be.ptr(done), C.byref(M) if met else None, be.stream)
        be.sync()
        if met:
            for k in met:
                metrics[k] = be.host(met[k]).copy()
        return be.host(state).copy(), be.host(obs).copy(), be.host(rew).copy(), be.host(done).copy()

    def close(self):
        self.be.lib.model_close(self.h)


class TwinStepper:
    """oracle.cpu_twin.Twin.step on the same records."""

    name = "twin"

    def __init__(self, cm):
        from oracle.cpu_twin import Twin

        self.cm, self.tw = cm, Twin(cm)
        tw = self.tw
        self.dims = nat.ModelDims(nq=tw.nq, nv=tw.nv, nu=tw.nu, nbody=tw.nbody, nefc=tw.nefc, obs_dim=tw.obs_dim, obs_pad=tw.obs_pad, rec_dim=tw.rec_dim,
                                  timestep=float(cm.t["timestep"]))
        tw.reset(1)
        self.reset_rec = tw.reset_rec.copy()

    def step(self, rec, action, n_frames, rc, metrics=None):
        from oracle.cpu_twin import Metrics, RewardCfg as TwinReward

        tw, N = self.tw, rec.shape[0]
        if tw.N != N:
            tw.reset(N)
        tw.state[...] = rec
        tw.obs[...] = np.nan
        tw.rc = TwinReward(*rc)
        a = np.ascontiguousarray(np.zeros((N, 1), f32) if tw.nu == 0 else action, f32)
        met = {k: np.ascontiguousarray(metrics[k], METRIC_TYPES[k]) for k in METRIC_TYPES} if metrics is not None else None
        M = Metrics(**{k: v.ctypes.data for k, v in met.items()}) if met else None
        tw.dll.twin_env_step(tw.h, N, n_frames, C.byref(tw.rc), tw.state.ctypes.data, tw.reset_rec.ctypes.data, a.ctypes.data, a.shape[1], tw.obs.ctypes.data, tw.obs_pad,
                             tw.reward.ctypes.data, tw.done.ctypes.data, C.byref(M) if met else None)
        if met:
            metrics.update(met)
        return tw.state.copy(), tw.obs.copy(), tw.reward.copy(), tw.done.copy()

    def close(self):
        self.tw.close()


def quaternion_joints(cm):
    """[(qpos address of the quaternion, dof address of its angular velocity)] of every free and ball joint."""
    out = []
    for j in range(cm.njnt):
        jt, qa, da = int(cm.t["jnt_type"][j]), int(cm.t["jnt_qposadr"][j]), int(cm.t["jnt_dofadr"][j])
        if jt == JNT_FREE:
            out.append((qa + 3, da + 3))
        elif jt == JNT_BALL:
            out.append((qa, da))
    return out


def fast_states(cm, N, seed):
    """States on which a subtly wrong integrator shows: walking_states with velocities put on top - every free and ball joint turning with
    |w| h in [0.1, 0.5], every other dof (a free joint's translation included) with |v| h in [0.01, 0.1], either sign.  Environment 0
    has w = 0 exactly on every quaternion joint (the integrator's `n > 0` branch); environment 1 stores its quaternions with norm
    1 +- 1e-3 (kinematics normalises on read, the integrator normalises what it writes) -> float32 qpos, qvel, ctrl, warm start."""
    assert N >= 3
    qpos, qvel, ctrl, warm = walking_states(cm, N, seed)
    rng = np.random.default_rng(1000 + seed)
    h = float(cm.t["timestep"])
    qvel = rng.uniform(0.01, 0.1, (N, cm.nv)) / h * rng.choice([-1.0, 1.0], (N, cm.nv))
    qpos = qpos.copy()
    for k, (qa, da) in enumerate(quaternion_joints(cm)):
        u = rng.standard_normal((N, 3))
        qvel[:, da:da + 3] = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.1, 0.5, (N, 1)) / h
        qvel[0, da:da + 3] = 0.0
        qpos[1, qa:qa + 4] *= 1.0 + (1e-3 if k % 2 == 0 else -1e-3)
    return qpos.astype(f32), qvel.astype(f32), ctrl.astype(f32), warm.astype(f32)


def position_bound(cm, qpos, qvel_new):
    """The float64 integration of float32 `qpos` with the float32 `qvel_new` and, per entry, how far a float32 kernel may be from it:
    max(4 x |float32 reference - float64 reference| on the same inputs, 2^-22 max(1, |q|)) - 4 x for a device's sinf / cosf / sqrtf of
    1 - 2 ulp where NumPy's are correctly rounded, the floor four float32 roundings of a unit-scale value.  Both from the reference.
    -> ref64, bound"""
    h = f32(cm.t["timestep"])
    r64 = integrate_positions(cm, qpos.astype(f64), qvel_new.astype(f64), float(h), f64)
    r32 = integrate_positions(cm, qpos.astype(f32), qvel_new.astype(f32), h, f32)
    return r64, np.maximum(4.0 * np.abs(r32.astype(f64) - r64), 2.0 ** -22 * np.maximum(1.0, np.abs(r64)))


def wrong_integrators(cm, qpos, qvel_old, qvel_new):
    """Three subtly wrong position updates in float64: the quaternion multiplied on the wrong side (w read in the world frame), a first-order
    quaternion update q + h/2 q (0, w) instead of the axis-angle one, positions advanced with the OLD velocity.  The first two are None for
    a robot without a quaternion joint."""
    h = float(f32(cm.t["timestep"]))
    q, v = qpos.astype(f64), qvel_new.astype(f64)
    good = integrate_positions(cm, q, v, h, f64)
    out = dict(world_frame=None, first_order=None, old_velocity=integrate_positions(cm, q, qvel_old.astype(f64), h, f64))
    qj = quaternion_joints(cm)
    if qj:
        wf, fo = good.copy(), good.copy()
        for qa, da in qj:
            w = v[:, da:da + 3]
            n = np.linalg.norm(w, axis=-1, keepdims=True)
            ax = w / np.where(n > 0, n, 1.0)
            dq = np.concatenate([np.cos(0.5 * n * h), ax * np.sin(0.5 * n * h)], -1)
            x = qmul(dq, q[:, qa:qa + 4])
            wf[:, qa:qa + 4] = x / np.linalg.norm(x, axis=-1, keepdims=True)
            x = q[:, qa:qa + 4] + 0.5 * h * qmul(q[:, qa:qa + 4], np.concatenate([np.zeros_like(n), w], -1))
            fo[:, qa:qa + 4] = x / np.linalg.norm(x, axis=-1, keepdims=True)
        out.update(world_frame=wf, first_order=fo)
    return out


def reward_from_records(cm, rec0, rec1, action, rc, n_frames, dims):
    """The reward of env.py:199-235 in float64 from the records themselves - |qpos0 - qpos| over all of qpos, z and com_x of the pre-step
    record, the action, com_x of the post-step record - and the budget of float32 roundings a kernel may be away from it:
    64 x 2^-24 x the sum of the weighted terms' magnitudes.  `rc`: the nine values of RewardCfg as float32 holds them.  -> reward, bound, clipped"""
    rc = [float(f32(x)) for x in rc]
    hmin, hmax, ec, sf, mdn, w_ctrl, w_pos, w_healthy, w_vel = rc
    nq, nv, OP = cm.nq, cm.nv, dims.obs_pad
    q = rec0[:, :nq].astype(f64)
    p0 = np.linalg.norm(np.asarray(cm.t["qpos0"], f32).astype(f64)[None] - q, axis=-1)
    e, cl = np.exp(-ec * p0), np.clip(p0, 0.0, mdn)
    z = q[:, 2]
    healthy = np.where((z < hmin) | (z > hmax), 0.0, 1.0)
    a = np.zeros((q.shape[0], 0)) if cm.nu == 0 else action.astype(f32).astype(f64)
    asq = np.sum(a * a, -1)
    dt_env = float(f32(f32(cm.t["timestep"]) * f32(n_frames)))
    vel = (rec1[:, OP + nv].astype(f64) - rec0[:, OP + nv].astype(f64)) / dt_env
    reward = -w_ctrl * asq + w_pos * (e - sf * cl) + w_vel * vel + w_healthy * healthy
    size = np.abs(w_ctrl) * asq + np.abs(w_pos) * (e + np.abs(sf) * cl) + np.abs(w_vel * vel) + np.abs(w_healthy) * healthy
    return reward, 64.0 * ULP32 * size, p0 > mdn


# ---------------------------------------------------------------------------------------------------------------------------------------
# bit-equality: instantiations, placements, the kernel compiled at start-up; reproducible training
# ---------------------------------------------------------------------------------------------------------------------------------------


def probe_and_steps(be, cm, seed=7, N=9, steps=6):
    """The forward probe on walking states and a stretch of env steps -> which kernel the handle runs (mppo_model_is_specialized), every output."""
    qpos, qvel, ctrl, warm = walking_states(cm, N, seed)
    q32 = [x.astype(f32) for x in (qpos, qvel, ctrl, warm)]
    h, dims, _keep = be.model(cm)
    flag = C.c_int32(-1)
    be.lib.model_is_specialized(h, C.byref(flag))
    got = probe(be, h, cm, *q32)
    OP, R = dims.obs_pad, dims.rec_dim
    state, reset_rec, obs = be.zeros((N, R)), be.zeros((R,)), be.zeros((N, OP))
    rew, done = be.zeros((N,)), be.zeros((N,), np.uint8)
    be.lib.env_reset(h, N, be.ptr(state), be.ptr(reset_rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), None, be.stream)
    rc = nat.RewardCfg(0.45, 2.0, 2.0, 0.2, 0.5, 0.1, 4.0, 1.0, 1.25)  # (a height band a biped leaves now and then: resets inside the stretch)
    r2 = np.random.default_rng(3)
    for _ in range(steps):
        act = be.arr((0.8 * r2.standard_normal((N, cm.nu))).astype(f32))
        be.lib.env_step(h, N, 2, C.byref(rc), be.ptr(state), be.ptr(reset_rec), be.ptr(act), cm.nu, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), None, be.stream)
        be.sync()
    got.update(state=be.host(state).copy(), obs=be.host(obs).copy(), rew=be.host(rew).copy(), done=be.host(done).copy())
    be.lib.model_close(h)
    return flag.value, got


def assert_bit_equal(a, b):
    for k in a:
        assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)), k


def startup_kernel_equals_runtime_sized(cm, tmp_path, monkeypatch, dims_check=None, N=300, steps=12):
    """The model's kernel compiled at start-up (minppo_amd/jit.py) against the run-time-sized one on the GPU, bit for bit over `steps` env steps:
    the path of tests/test_jit.py::test_attached_kernel_equals_the_runtime_sized_kernel.  Both handles start on the run-time-sized kernel
    (an instantiation of the library's own is bypassed) and the compiled code object is attached to the second.  `dims_check(dims)` holds
    what the test expects of the kernel's compile-time dimensions."""
    import torch

    from minppo_amd import jit

    monkeypatch.setenv(jit.CACHE_ENV, str(tmp_path))
    lib = nat.load()
    dims_ = jit.dims_of(cm)
    assert dims_check is None or dims_check(dims_)
    image = jit.compile_kernel(dims_, 48).read_bytes()
    blob = np.frombuffer(cm.to_blob(), np.uint8)
    dblob = torch.from_numpy(blob.copy()).cuda()
    outs = []
    for attach in (False, True):
        monkeypatch.setenv("MPPO_ENV_GENERIC", "1")
        h = C.c_void_p()
        lib.model_open(blob.ctypes.data, blob.size, dblob.data_ptr(), C.byref(h))
        monkeypatch.delenv("MPPO_ENV_GENERIC")
        if attach:
            assert jit.attach(lib, h, image, 48)
            kind = C.c_int32(-1)
            lib.model_is_specialized(h, C.byref(kind))
            assert kind.value == 2
        dims = nat.ModelDims()
        lib.model_get_dims(h, C.byref(dims))
        assert dims.lds_bytes <= 160 * 1024
        outs.append((h, run_steps(lib, h, dims, N, steps, torch)))
    for t, (a, b) in enumerate(zip(outs[0][1], outs[1][1])):
        for x, y, what in zip(a, b, ("state", "observation", "reward", "done")):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what} differs at step {t}"
    for h, _ in outs:
        lib.model_close(h)


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def leaves(tree):
    if isinstance(tree, dict):
        return [x for k in sorted(tree) for x in leaves(tree[k])]
    if isinstance(tree, (list, tuple)):
        return [x for v in tree for x in leaves(v)]
    return [tree]


def trains_reproducibly(model, trainer=False):
    """Two training runs on `model` (environment.model=...) with one seed end in bit-identical, finite parameters.  make_train: four updates at
    512 environments, finite episode metrics too; trainer=True: the Trainer itself, five updates at 1024 environments."""
    import torch

    from minppo_amd.config import load_config_from_cli
    from minppo_amd.train import Trainer, make_train

    small = ["training.num_envs=512", "training.num_minibatches=4", "training.update_epochs=2", "training.total_timesteps=20480"]
    large = ["training.num_envs=1024", "training.num_minibatches=4", "training.update_epochs=2", "training.total_timesteps=1000000"]
    flat = []
    for _ in range(2):
        cfg = load_config_from_cli(["stompy_pro", f"environment.model={model}", *(large if trainer else small)])
        if trainer:
            tr = Trainer(cfg)
            tr.reset()
            for _ in range(5):
                tr.update()
            torch.cuda.synchronize()
            flat.append(tr.params_flat())
            tr.close()
            continue
        o = make_train(cfg)(1337, log_every=1)
        flat.append(np.concatenate([host(x).reshape(-1).astype(f32) for x in leaves(o.runner_state.train_state.params)]))
        assert len(o.metrics["mean_reward"]) == 4
        for k in ("mean_reward", "done_fraction", "mean_episode_return", "mean_episode_length", "total_loss"):
            assert np.isfinite(np.asarray(o.metrics[k], f64)).all(), k
    assert flat[0].size > 0 and np.isfinite(flat[0]).all()
    assert np.array_equal(flat[0].view(np.uint8), flat[1].view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the oracle's recording on the committed models: a feature a model does not use changes nothing for it
# ---------------------------------------------------------------------------------------------------------------------------------------


def feature_models():
    """(name, maker) of every built-in robot and every fixture file: the models of tests/golden/oracle_features.npz."""
    out = [(n, lambda f=f: compile_model(f())) for n, f in sorted(BUILTIN_MODELS.items())]
    files = list(GOLDEN.glob("*.xml")) + [GOLDEN / "export_biped" / "robot.xml", GOLDEN / "many_dofs" / "hands_humanoid.xml"]
    files += list((GOLDEN / "equality").glob("*.xml")) + list((GOLDEN / "ball_joints").glob("*.xml"))
    return out + [(str(p.relative_to(GOLDEN)), lambda p=p: load_model(str(p))) for p in sorted(files)]


def feature_record(cm):
    """What the recording holds of one model: three environments from qpos0 with random velocities and controls (seed 11), a forward pass and
    two steps of the float64 oracle; efc_J contracted with cos(0 .. nv - 1)."""
    rng = np.random.default_rng(11)
    N = 3
    q = np.tile(np.asarray(cm.t["qpos0"], f64), (N, 1))
    v = 0.1 * rng.standard_normal((N, cm.nv))
    ctrl = 0.5 * rng.standard_normal((N, cm.nu))
    ph = Physics(cm.t)
    d = ph.pipeline_init(q, v)
    for _ in range(2):
        d = ph.pipeline_step(d, ctrl)
    out = {k: np.asarray(d[k]) for k in ("qpos", "qvel", "qacc", "efc_D", "efc_aref", "qfrc_actuator", "qfrc_passive")}
    out["efc_J_cos"] = np.einsum("nrv,v->nr", d.efc_J, np.cos(np.arange(cm.nv, dtype=f64)))
    return out


def assert_oracle_reproduces_the_recording(names):
    """oracle.physics_oracle.Physics against tests/golden/oracle_features.npz, recorded from the oracle as it was when per-row contact
    parameters, equalities and ball joints were three subclasses stacked on it (the unified class equalled that tower value for value,
    profiles/oracle_unification_equality.txt).  Tolerances of test_oracle_reproduces_physics_golden: qpos 1e-11 absolute; every other
    quantity 1e-9 (its observation, which holds qvel and qfrc_actuator) of max |recorded| + 1e-6 - efc_D reaches 1e5, where an absolute
    1e-9 is below float64 rounding.  On the machine that recorded it the difference is zero."""
    want = np.load(GOLDEN / "oracle_features.npz")
    makers = dict(feature_models())
    for name in names:
        for k, got in feature_record(makers[name]()).items():
            w = want[f"{name}/{k}"]
            assert got.shape == w.shape, (name, k)
            if w.size:  # (a model without constraint rows records empty efc arrays)
                err = np.abs(got - w).max()
                assert err <= (1e-11 if k == "qpos" else 1e-9 * (np.abs(w).max() + 1e-6)), (name, k, err)
