"""Domain randomisation: per-environment friction, actuator gain and payload in the environment kernel (csrc/k_physics.hip KMODE 6 .. 8), the stateless draw
(csrc/domrand.h, k_domrand.hip), the engine (`mppo_engine_set_domain`), the evaluator (`mppo_evaluate_domain`) and the Python surface
(`environment.friction_scale_*` / `actuator_scale_*` / `added_mass_*`, `HumanoidEnv.reset(domain=)`).

1. the fill, bit for bit against `jaxrng.domain_params_philox`      5. specialised / run-time-sized / out-of-LDS / start-up-compiled kernels under a table
2. the identity table (1, 1, 0, 0): the unrandomised entry points   6. the engine: composition, graph = eager, checkpoint / resume, off is off, call order
3. THE CONTRACT: environment n = the unrandomised kernels on the    7. the evaluator's composition, evaluate(), config keys, HumanoidEnv, the command line
   model whose tables are replaced by row n, bit for bit
4. the forward probe against the float64 oracle on replaced tables

The reference of 3 is the library's own unrandomised entry points on `_replaced(cm, row, body)` - a copy of the compiled model whose con_friction, act_gain,
act_bias and body_mass hold the float32 products / sums - re-blobbed; of 4, `Physics` on the same tables.  Sizes: N = 37 for the draw, 7 for the physics -
no multiple of the four environments of a wave, more than one wave."""

import copy
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
from minppo_amd.config import make_config
from minppo_amd.model import JNT_BALL, load_model
from oracle.physics_oracle import Physics, PhysState
from physics_harness import GOLDEN, METRIC_TYPES, SMOOTH_TOL

f32, f64 = np.float32, np.float64
ROOT = Path(__file__).resolve().parent.parent
BASE = {"kscale_id": "5eb3cb7f23232298", "visualization": {"camera_name": "track"}}
SEED = 5
RANGES = dict(friction=(0.3, 1.7), actuator=(0.6, 1.4), mass=(-0.5, 4.0))

# the hand-picked rows of the contract: friction 0.25 .. 2.0, actuator 0.5 .. 1.5, mass -1 .. +5 kg, one identity row (row 2)
ROWS = np.array([[0.25, 1.5, 5.0, 0.0],
                 [2.0, 0.5, -1.0, 0.0],
                 [1.0, 1.0, 0.0, 0.0],
                 [0.6, 1.25, 2.5, 0.0],
                 [1.0, 0.8, 0.0, 0.0],
                 [1.3, 1.0, -0.4, 0.0],
                 [0.25, 0.5, 5.0, 0.0]], f32)

ROBOTS = {"pro": lambda: load_model("synth_stompy_pro"),                                          # a library instantiation
          "ball_humanoid": lambda: load_model(str(GOLDEN / "ball_joints" / "ball_humanoid.xml")),  # a motor on a ball joint
          "contact_params": lambda: load_model(str(GOLDEN / "contact_params_humanoid.xml")),       # per-row parameters, condim 1
          "export_biped": lambda: load_model(str(GOLDEN / "export_biped" / "robot.xml"))}         # matrices in global memory
_CM = {}


def _cm(which):
    if which not in _CM:
        _CM[which] = ROBOTS[which]()
    return _CM[which]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _dcfg(friction=RANGES["friction"], actuator=RANGES["actuator"], mass=RANGES["mass"], body=1, seed=SEED, rank=0):
    return nat.DomainCfg(friction[0], friction[1], actuator[0], actuator[1], mass[0], mass[1], body, seed, rank)


def _fill(be, cfg, N):
    out = be.full((N, 4), np.nan)
    be.lib.domain_fill(C.byref(cfg), N, be.ptr(out), be.stream)
    be.sync()
    return be.host(out).copy()


def _leaf(cm):
    """The deepest body of the tree (the last of them): a leaf."""
    parent = [int(x) for x in cm.t["body_parent"]]
    depth = [0] * cm.nbody
    for b in range(1, cm.nbody):
        depth[b] = depth[parent[b]] + 1
    leaf = max(range(cm.nbody), key=lambda b: (depth[b], b))
    assert leaf not in parent
    return leaf


def _rows_for(cm, body):
    """ROWS with the payload kept physical on `body`: a body lighter than 2 kg loses at most half its mass (on the robots' roots the rows are ROWS)."""
    rows = ROWS.copy()
    m = f32(cm.t["body_mass"][body])
    if m < 2.0:
        rows[:, 2] = np.maximum(rows[:, 2], f32(-0.5) * m)
    return rows


def _replaced(cm, row, body):
    """The compiled model whose tables are replaced as the header's "Semantics" say, each value formed in float32."""
    fs, as_, dm = (f32(x) for x in row[:3])
    t = dict(cm.t)
    fr = np.array(t["con_friction"], f64).reshape(-1, 3).copy()
    fr[:, 0] = (fr[:, 0].astype(f32) * fs).astype(f64)
    t["con_friction"] = fr.reshape(np.shape(t["con_friction"]))
    t["act_gain"] = (np.asarray(t["act_gain"]).astype(f32) * as_).astype(f64)
    bias = np.array(t["act_bias"], f64).reshape(-1, 3).copy()
    for u in range(cm.nu):
        on_ball = int(t["jnt_type"][int(t["dof_jntid"][int(t["act_dofid"][u])])]) == JNT_BALL
        if not on_ball:
            bias[u] = (bias[u].astype(f32) * as_).astype(f64)
    t["act_bias"] = bias.reshape(np.shape(t["act_bias"]))
    mass = np.array(t["body_mass"], f64).copy()
    mass[body] = f64(f32(mass[body]) + dm)
    t["body_mass"] = mass
    out = copy.copy(cm)
    out.t = t
    return out


class Run:
    """A reset and T env steps through the unrandomised entry points (table None) or the randomised ones, with every restart the way the engine does it:
    unrandomised - the step's copy of the reset record, then mppo_env_reinit over done when reset noise is on; randomised - mppo_env_reset_domain over done."""

    def __init__(self, be, cm, N, rc, table=None, mass_body=1, noise=0.0, n_frames=2):
        self.be, self.cm, self.N, self.noise, self.n_frames, self.mass_body = be, cm, N, noise, n_frames, mass_body
        self.h, self.dims, self._keep = be.model(cm)
        OP, R = self.dims.obs_pad, self.dims.rec_dim
        self.state, self.reset_rec, self.obs = be.zeros((N, R)), be.zeros((R,)), be.full((N, OP), np.nan)
        self.rew, self.done = be.zeros((N,)), be.zeros((N,), np.uint8)
        self.met = {k: be.full((N,), 7, dt) for k, dt in METRIC_TYPES.items()}
        self.Ms = nat.EnvMetrics(**{k: be.ptr(v) for k, v in self.met.items()})
        self.rc = nat.RewardCfg(*rc)
        self.table = be.arr(np.asarray(table, f32)) if table is not None else None
        self.t = 0
        lib, p = be.lib, be.ptr
        if self.table is None:
            lib.env_reset(self.h, N, p(self.state), p(self.reset_rec), p(self.obs), OP, p(self.rew), p(self.done), C.byref(self.Ms), be.stream)
            if noise > 0:
                lib.env_reinit(self.h, N, p(self.state), p(self.obs), OP, None, noise, 0, SEED, 0, None, None, 0, be.stream)
        else:
            lib.env_reset_domain(self.h, N, p(self.state), p(self.reset_rec), p(self.obs), OP, p(self.rew), p(self.done), C.byref(self.Ms), None, p(self.table),
                                 mass_body, 0.0, 0, SEED, 0, None, None, 0, be.stream)
            if noise > 0:
                lib.env_reset_domain(self.h, N, p(self.state), None, p(self.obs), OP, None, None, None, None, p(self.table), mass_body, noise, 0, SEED, 0, None,
                                     None, 0, be.stream)
        be.sync()

    def snapshot(self):
        be = self.be
        out = dict(state=be.host(self.state).copy(), obs=be.host(self.obs).copy(), rew=be.host(self.rew).copy(), done=be.host(self.done).copy())
        out.update({k: be.host(v).copy() for k, v in self.met.items()})
        return out

    def step(self, action, push_body=0, xfrc=None):
        be, lib, p, N, OP, nu = self.be, self.be.lib, self.be.ptr, self.N, self.dims.obs_pad, max(self.cm.nu, 1)
        a = be.arr(action.astype(f32))
        x = be.arr(xfrc.astype(f32)) if xfrc is not None else None
        self.t += 1
        if self.table is None:
            lib.env_step_xfrc(self.h, N, self.n_frames, C.byref(self.rc), p(self.state), p(self.reset_rec), p(a), nu, p(self.obs), OP, p(self.rew), p(self.done),
                              C.byref(self.Ms), push_body, p(x), be.stream)
            if self.noise > 0:
                lib.env_reinit(self.h, N, p(self.state), p(self.obs), OP, p(self.done), self.noise, 0, SEED, 0, None, None, self.t, be.stream)
        else:
            lib.env_step_domain(self.h, N, self.n_frames, C.byref(self.rc), p(self.state), p(self.reset_rec), p(a), nu, p(self.obs), OP, p(self.rew), p(self.done),
                                C.byref(self.Ms), push_body, p(x), p(self.table), self.mass_body, be.stream)
            lib.env_reset_domain(self.h, N, p(self.state), None, p(self.obs), OP, None, None, None, p(self.done), p(self.table), self.mass_body, self.noise, 0,
                                 SEED, 0, None, None, self.t, be.stream)
        be.sync()
        return self.snapshot()

    def close(self):
        self.be.lib.model_close(self.h)


# half-widths of the height window about qpos0's height that each robot, as the file describes it, leaves after three to six of the eight steps of two frames
# under the random controls below (measured on the unrandomised robots): episodes end inside a short run, and not at every step
BAND = {"pro": 5e-4, "ball_humanoid": 4e-3, "contact_params": 1.2e-2, "export_biped": 2e-3}


def _band(cm):
    z0, w = float(cm.t["qpos0"][2]), BAND[next(k for k in ROBOTS if _CM.get(k) is cm)]
    return (z0 - w, z0 + w, 2.0, 0.2, 0.5, 0.1, 4.0, 1.0, 1.25)


def _actions(cm, N, T, seed=3):
    return (0.8 * np.random.default_rng(seed).standard_normal((T, N, max(cm.nu, 1)))).astype(f32)


def _rollout(run, actions, push_body=0, xfrc=None):
    out = [run.snapshot()]
    for t in range(actions.shape[0]):
        out.append(run.step(actions[t], push_body, None if xfrc is None else xfrc[t]))
    run.close()
    return out


def _probe_d(be, h, cm, q32, table, mass_body, push_body=0, xfrc=None):
    """ph.probe through mppo_physics_forward_domain."""
    N = q32[0].shape[0]
    nv, nb, nefc = cm.nv, cm.nbody, max(cm.nefc, 1)
    shapes = dict(qM=(N, nv, nv), qfrc_bias=(N, nv), qfrc_passive=(N, nv), qfrc_actuator=(N, nv), qacc_smooth=(N, nv), efc_J=(N, nefc, nv), efc_D=(N, nefc),
                  efc_aref=(N, nefc), qacc=(N, nv), cinert=(N, nb, 10), cvel=(N, nb, 6), subtree_com1=(N,), xpos=(N, nb, 3), qacc_euler=(N, nv))
    out = {k: be.zeros(s) for k, s in shapes.items()}
    niter = be.zeros((N,), np.int32)
    d_in = [be.arr(x.astype(f32)) for x in q32]
    x = be.arr(xfrc.astype(f32)) if xfrc is not None else None
    tab = be.arr(np.asarray(table, f32))
    pr = nat.ForwardProbe(**{k: be.ptr(v) for k, v in out.items()}, solver_niter=be.ptr(niter))
    be.lib.physics_forward_domain(h, N, be.ptr(d_in[0]), be.ptr(d_in[1]), be.ptr(d_in[2]) if cm.nu else 0, be.ptr(d_in[3]), C.byref(pr), push_body, be.ptr(x),
                                  be.ptr(tab), mass_body, be.stream)
    be.sync()
    res = {k: be.host(v).copy() for k, v in out.items()}
    res["niter"] = be.host(niter).copy()
    return res


# ---- 1: the fill ------------------------------------------------------------------------------------------------------------------------------------------


def test_fill_equals_the_host_restatement(be):
    N = 37
    for seed in (SEED, 2 ** 40 + 11):
        got = _fill(be, _dcfg(seed=seed), N)
        want = jaxrng.domain_params_philox(seed, 0, N, **RANGES)
        assert np.array_equal(_bits(got), _bits(want)), seed
        for k, (lo, hi) in enumerate(RANGES.values()):
            assert (got[:, k] >= f32(lo)).all() and (got[:, k] <= f32(hi)).all(), (k, got[:, k].min(), got[:, k].max())
            assert got[:, k].max() - got[:, k].min() > 0.5 * (hi - lo)  # (37 draws cover more than half the range)
        assert (_bits(got[:, 3]) == 0).all()
    a, b = _fill(be, _dcfg(rank=0), N), _fill(be, _dcfg(rank=1), N)
    assert not np.array_equal(a, b) and (a[:, :3] != b[:, :3]).all(1).sum() > N // 2
    assert np.array_equal(_bits(b), _bits(jaxrng.domain_params_philox(SEED, 1, N, **RANGES)))
    assert not np.array_equal(_fill(be, _dcfg(seed=SEED + 1), N), a)
    # min == max: exactly that value, whatever the bits drawn
    fixed = _fill(be, _dcfg(friction=(0.3, 0.3), actuator=(1.1, 1.1), mass=(5.0, 5.0)), N)
    assert np.array_equal(_bits(fixed), _bits(np.tile(np.array([0.3, 1.1, 5.0, 0.0], f32), (N, 1))))
    assert np.array_equal(_bits(fixed), _bits(jaxrng.domain_params_philox(SEED, 0, N, (0.3, 0.3), (1.1, 1.1), (5.0, 5.0))))
    ident = _fill(be, _dcfg(friction=(1, 1), actuator=(1, 1), mass=(0, 0)), N)
    assert np.array_equal(_bits(ident), _bits(np.tile(np.array([1, 1, 0, 0], f32), (N, 1))))


def test_fill_refuses_bad_configurations(be):
    out = be.zeros((4, 4))
    f = be.lib._fn["mppo_domain_fill"]
    for bad, word in ((_dcfg(friction=(0.9, 0.5)), "friction_min"), (_dcfg(actuator=(1.5, 0.5)), "actuator_min"), (_dcfg(mass=(1.0, 0.0)), "mass_min"),
                      (_dcfg(friction=(-0.1, 1.0)), "negative"), (_dcfg(actuator=(-1.0, 1.0)), "negative"), (_dcfg(rank=300), "rank"), (_dcfg(rank=-1), "rank"),
                      (_dcfg(friction=(float("nan"), 1.0)), "friction_min")):
        assert f(C.byref(bad), 4, be.ptr(out), be.stream) != 0 and word in be.lib.last_error(), word
    assert f(C.byref(_dcfg()), 4, 0, be.stream) != 0 and "null table" in be.lib.last_error()
    with pytest.raises(ValueError):
        jaxrng.domain_params_philox(SEED, 0, 4, friction=(0.9, 0.5))
    with pytest.raises(ValueError):
        jaxrng.domain_params_philox(SEED, 0, 4, actuator=(-0.5, 0.5))


def test_entry_points_refuse_a_null_table_and_a_wrong_body(be):
    cm = _cm("pro")
    h, dims, _keep = be.model(cm)
    N, OP, R, nu = 5, dims.obs_pad, dims.rec_dim, cm.nu
    state, rr, obs, rew, done, act = be.zeros((N, R)), be.zeros((R,)), be.zeros((N, OP)), be.zeros((N,)), be.zeros((N,), np.uint8), be.zeros((N, nu))
    tab = be.arr(np.tile(np.array([1, 1, 0, 0], f32), (N, 1)))
    rc = nat.RewardCfg(*_band(cm))
    p = be.ptr
    reset, step, fwd = (be.lib._fn[k] for k in ("mppo_env_reset_domain", "mppo_env_step_domain", "mppo_physics_forward_domain"))
    q = [be.zeros((N, cm.nq)), be.zeros((N, cm.nv)), be.zeros((N, nu)), be.zeros((N, cm.nv))]
    pr = nat.ForwardProbe()
    for table, body, word in ((None, 1, "null table"), (tab, 0, "mass_body"), (tab, cm.nbody, "mass_body"), (tab, -3, "mass_body")):
        assert reset(h, N, p(state), p(rr), p(obs), OP, p(rew), p(done), None, None, p(table), body, 0.0, 0, SEED, 0, None, None, 0, be.stream) != 0
        assert word in be.lib.last_error()
        assert step(h, N, 1, C.byref(rc), p(state), p(rr), p(act), nu, p(obs), OP, p(rew), p(done), None, 0, None, p(table), body, be.stream) != 0
        assert word in be.lib.last_error()
        assert fwd(h, N, p(q[0]), p(q[1]), p(q[2]), p(q[3]), C.byref(pr), 0, None, p(table), body, be.stream) != 0
        assert word in be.lib.last_error()
    # a wrench on a body the model does not have
    x = be.zeros((N, 6))
    assert step(h, N, 1, C.byref(rc), p(state), p(rr), p(act), nu, p(obs), OP, p(rew), p(done), None, cm.nbody, p(x), p(tab), 1, be.stream) != 0
    assert "push body" in be.lib.last_error()
    be.lib.model_close(h)


# ---- 2: the identity table --------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("which", ["pro", "ball_humanoid"])
def test_the_identity_table_changes_no_bit(be, which):
    cm = _cm(which)
    N, T = 7, 6
    ident = np.tile(np.array([1, 1, 0, 0], f32), (N, 1))
    acts = _actions(cm, N, T)
    plain = _rollout(Run(be, cm, N, _band(cm)), acts)
    rand = _rollout(Run(be, cm, N, _band(cm), table=ident, mass_body=_leaf(cm)), acts)
    assert sum(int(s["done"].sum()) for s in plain) > 0  # (the masked re-initialisation ran)
    for t, (a, b) in enumerate(zip(plain, rand)):
        for k in a:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (which, t, k)
    qpos, qvel, ctrl, warm = ph.walking_states(cm, N, 11)
    q32 = [x.astype(f32) for x in (qpos, qvel, ctrl, warm)]
    h, dims, _keep = be.model(cm)
    want = ph.probe(be, h, cm, *q32)
    be.sync()
    want = {k: np.array(v) for k, v in want.items()}
    ph.assert_bit_equal(want, _probe_d(be, h, cm, q32, ident, 1))
    be.lib.model_close(h)


# ---- 3: the contract --------------------------------------------------------------------------------------------------------------------------------------

_REF = {}


def _reference(be, which, body_kind, variant, N, T):
    """Environment n of the unrandomised entry points on the model replaced by row n, from the shared actions: computed once per backend and case."""
    key = (be.name, which, body_kind, variant)
    if key not in _REF:
        cm = _cm(which)
        body = 1 if body_kind == "root" else _leaf(cm)
        rows = _rows_for(cm, body)
        acts = _actions(cm, N, T)
        xfrc, push_body, noise = _variant(cm, variant, N, T)
        per_env = []
        for n in range(N):
            run = _rollout(Run(be, _replaced(cm, rows[n], body), N, _band(cm), noise=noise), acts, push_body, xfrc)
            per_env.append([{k: v[n].copy() for k, v in s.items()} for s in run])
        _REF[key] = (cm, body, rows, acts, xfrc, push_body, noise, per_env)
    return _REF[key]


def _variant(cm, variant, N, T):
    if variant == "xfrc":
        rng = np.random.default_rng(17)
        x = np.concatenate([rng.uniform(-60, 60, (T, N, 3)), rng.uniform(-4, 4, (T, N, 3))], 2).astype(f32)
        x[:, 2] = 0.0  # (an all-zero row: the unpushed bits)
        return x, _leaf(cm), 0.0
    return None, 0, (0.3 * BAND[next(k for k in ROBOTS if _CM.get(k) is cm)] if variant == "noise" else 0.0)  # (reset noise well inside the height window)


CASES = [(w, b, "plain") for w in ROBOTS for b in ("root", "leaf")] + [("pro", "leaf", "xfrc"), ("ball_humanoid", "root", "xfrc"), ("pro", "root", "noise"),
                                                                        ("export_biped", "leaf", "noise")]


@pytest.mark.parametrize("which,body_kind,variant", CASES)
def test_environment_n_is_the_unrandomised_kernel_on_the_replaced_model(be, which, body_kind, variant):
    N, T = len(ROWS), 8
    cm, body, rows, acts, xfrc, push_body, noise, ref = _reference(be, which, body_kind, variant, N, T)
    # from the reference runs alone: an episode ends inside the run (the re-initialisation path), the rows differ from one another and from the plain robot
    ended = np.array([[int(s["done"]) for s in ref[n][1:]] for n in range(N)])
    print(f"{which} / {body_kind} / {variant}: episodes ended per environment {ended.sum(1)} of {T} steps")
    assert ended.sum() >= 1 and (ended.sum(1) < T).any()
    hist = [np.concatenate([s["state"] for s in ref[n]]) for n in range(N)]
    assert len({_bits(x).tobytes() for x in hist}) == N  # (seven different robots: no two rows give the same records)
    got = _rollout(Run(be, cm, N, _band(cm), table=rows, mass_body=body, noise=noise), acts, push_body, xfrc)
    for t in range(T + 1):
        for n in range(N):
            for k, want in ref[n][t].items():
                assert np.array_equal(_bits(got[t][k][n]), _bits(want)), (which, body_kind, variant, "step", t, "environment", n, k)


# ---- 4: the forward probe against the float64 oracle on the replaced tables -----------------------------------------------------------------------------

ROW_TOL = dict(efc_J=1e-5, efc_D=5e-4, efc_aref=5e-4)  # (tests/physics_harness.py check_against_oracle's callers: the kernel's rows against the oracle's, of each one's scale)
# seeds of walking_states for which at least half the environments are well-conditioned (oracle_pair), every distinct row has one that is, and an environment with a
# scaled friction is in contact - chosen from the oracle alone (the ball-joint humanoid starts above the floor: seeds 11 and 12 leave all eight in the air)
ORACLE_SEEDS = {"pro": 11, "ball_humanoid": 13, "contact_params": 11, "export_biped": 11}


@pytest.mark.parametrize("which", list(ROBOTS))
def test_forward_probe_follows_the_oracle_on_the_replaced_tables(be, which):
    cm = _cm(which)
    N = 8
    body = _leaf(cm) if which in ("pro", "contact_params") else 1
    rows = _rows_for(cm, body)[[0, 1, 3, 5]]
    table = np.repeat(rows, 2, 0)  # (four distinct rows, two environments each: eight environments, two waves)
    qpos, qvel, ctrl, warm = ph.walking_states(cm, N, ORACLE_SEEDS[which])
    q32 = [x.astype(f32) for x in (qpos, qvel, ctrl if cm.nu else np.zeros((N, 1)), warm)]
    refs, goods = [], np.zeros(N, bool)
    for r in range(4):
        ref, _ref32, good, scale = ph.oracle_pair(_replaced(cm, rows[r], body), q32)
        refs.append((ref, scale))
        goods[2 * r:2 * r + 2] = good[2 * r:2 * r + 2]
    assert goods.sum() >= N // 2, (which, goods)  # from the oracle alone, before the kernel is looked at
    assert all(goods[2 * r:2 * r + 2].any() for r in range(4)), (which, goods)  # ... and every distinct row has a well-conditioned environment: no row's check is empty
    # (from the oracle alone too) the environments in contact, and that the friction scale moves their rows: the oracle on the file's robot against the oracle on the row's
    ref_plain, _p32, _pg, _ps = ph.oracle_pair(cm, q32)
    touching = np.array([bool((refs[n // 2][0].efc_D[n, cm.neq + cm.nlimit:] > 0).any()) for n in range(N)]) if cm.ncon else np.zeros(N, bool)
    scaled = np.array([rows[n // 2][0] != 1.0 for n in range(N)])
    assert (touching & scaled).any(), (which, touching)
    h, dims, _keep = be.model(cm)
    got = _probe_d(be, h, cm, q32, table, body)
    plain = ph.probe(be, h, cm, *q32)
    be.sync()
    be.lib.model_close(h)
    for r, (ref, scale) in enumerate(refs):
        env = slice(2 * r, 2 * r + 2)
        for k, tol in list(SMOOTH_TOL.items()) + [("cinert", SMOOTH_TOL["qM"]), ("qfrc_actuator", SMOOTH_TOL["qfrc_bias"])]:
            want = ref[k]
            if want.size:
                err = np.abs(got[k].reshape(want.shape)[env] - want[env]).max() / scale(k)
                print(f"{which} row {r} {k}: err {err:.3e} (tolerance {tol:.0e})")
                assert err <= tol, (which, r, k, err)
        if cm.nefc:
            g = goods[env]
            gD = got["efc_D"].reshape(N, -1)[env]
            assert ((gD > 0) == (ref.efc_D[env] > 0))[g].all(), (which, r)
            for k, tol in ROW_TOL.items():
                want = ref[k]
                err = np.abs(got[k].reshape(want.shape)[env][g] - want[env][g]).max() / scale(k)
                print(f"{which} row {r} {k}: err {err:.3e} (tolerance {tol:.0e})")
                assert err <= tol, (which, r, k, err)
    # the rows do something: the mass moves cinert and qM, the actuator scale qfrc_actuator, the friction the contact rows of an environment in contact
    assert not np.array_equal(got["cinert"], np.array(plain["cinert"])) and not np.array_equal(got["qM"], np.array(plain["qM"]))
    if cm.nu:
        assert not np.array_equal(got["qfrc_actuator"], np.array(plain["qfrc_actuator"]))
    for n in np.flatnonzero(touching & scaled):  # a scaled friction moves the contact rows of an environment in contact, in the kernel as in the oracle
        assert not np.array_equal(refs[n // 2][0].efc_J[n], ref_plain.efc_J[n]) and not np.array_equal(refs[n // 2][0].efc_D[n], ref_plain.efc_D[n]), (which, n)
        assert not np.array_equal(got["efc_J"][n], np.array(plain["efc_J"])[n]) and not np.array_equal(got["efc_D"][n], np.array(plain["efc_D"])[n]), (which, n)


# ---- 5: placement changes nothing -------------------------------------------------------------------------------------------------------------------------


def _random_steps(be, cm, N=9, steps=6, want_kind=None):
    """A randomised reset, the probe and six randomised steps (a wrench on the leaf, restarts through the reset kernel) -> every output."""
    body = _leaf(cm)
    table = jaxrng.domain_params_philox(SEED, 0, N, friction=(0.25, 2.0), actuator=(0.5, 1.5), mass=(float(_rows_for(cm, body)[:, 2].min()), 3.0))
    run = Run(be, cm, N, _band(cm), table=table, mass_body=body)
    if want_kind is not None:
        flag = C.c_int32(-1)
        be.lib.model_is_specialized(run.h, C.byref(flag))
        assert flag.value == want_kind
    qpos, qvel, ctrl, warm = ph.walking_states(cm, N, 11)
    q32 = [x.astype(f32) for x in (qpos, qvel, ctrl, warm)]
    out = {"probe_" + k: v for k, v in _probe_d(be, run.h, cm, q32, table, body).items()}
    rng = np.random.default_rng(3)
    ended = 0
    for t in range(steps):
        x = np.concatenate([rng.uniform(-50, 50, (N, 3)), rng.uniform(-5, 5, (N, 3))], 1).astype(f32)
        snap = run.step((0.8 * rng.standard_normal((N, max(cm.nu, 1)))).astype(f32), body, x)
        ended += int(snap["done"].sum())
        out.update({f"{k}_{t}": v for k, v in snap.items()})
    run.close()
    assert ended > 0
    return out


def test_randomised_steps_are_the_same_bits_under_every_placement(be, monkeypatch):
    """As tests/test_push.py::test_pushed_steps_are_the_same_bits_under_every_placement: the library's instantiation, the run-time-sized kernel and the matrices
    in LDS / in global memory, under a table."""
    for which in ("pro", "export_biped"):
        cm = _cm(which)
        monkeypatch.delenv("MPPO_ENV_GENERIC", raising=False)
        monkeypatch.delenv("MPPO_ENV_SPILL", raising=False)
        spec = _random_steps(be, cm, want_kind=1)
        assert np.isfinite(spec["state_5"]).all()
        monkeypatch.setenv("MPPO_ENV_GENERIC", "1")
        ph.assert_bit_equal(spec, _random_steps(be, cm, want_kind=0))
        monkeypatch.delenv("MPPO_ENV_GENERIC")
        if which == "export_biped":
            for spill in ("0", "1", "3"):
                monkeypatch.setenv("MPPO_ENV_SPILL", spill)
                ph.assert_bit_equal(spec, _random_steps(be, cm, want_kind=0))
            monkeypatch.delenv("MPPO_ENV_SPILL")


@pytest.mark.gpu
def test_kernel_compiled_at_start_up_equals_the_runtime_sized_kernel_under_a_table(tmp_path, monkeypatch):
    """environment.jit_kernel's code object for the ball-joint humanoid (the run-time-sized kernel forced, then the code object attached) under a table."""
    import torch  # noqa: F401

    from backends import get_backend
    from minppo_amd import jit

    be = get_backend("hip")
    cm = _cm("ball_humanoid")
    monkeypatch.setenv(jit.CACHE_ENV, str(tmp_path))
    monkeypatch.delenv("MPPO_TEST_JIT", raising=False)
    image = jit.compile_kernel(jit.dims_of(cm), 48).read_bytes()
    orig = be.model

    def generic(cm_, include_c_vals=True):
        monkeypatch.setenv("MPPO_ENV_GENERIC", "1")
        try:
            return orig(cm_, include_c_vals)
        finally:
            monkeypatch.delenv("MPPO_ENV_GENERIC")

    def attached(cm_, include_c_vals=True):
        h, dims, keep = generic(cm_, include_c_vals)
        assert jit.attach(be.lib, h, image, 48)
        be.lib.model_get_dims(h, C.byref(dims))
        return h, dims, keep

    monkeypatch.setattr(be, "model", generic)
    want = _random_steps(be, cm, want_kind=0)
    monkeypatch.setattr(be, "model", attached)
    ph.assert_bit_equal(want, _random_steps(be, cm, want_kind=2))


# ---- 6: the engine ----------------------------------------------------------------------------------------------------------------------------------------

ENGINE = ["training.num_envs=32", "training.num_steps=3", "rl.num_env_steps=3", "training.num_minibatches=2", "training.update_epochs=1", "model.hidden_size=32",
          "training.total_timesteps=100000", "training.rng_impl=philox"]
RANDOMISED = ["environment.friction_scale_min=0.3", "environment.friction_scale_max=1.7", "environment.actuator_scale_min=0.6", "environment.actuator_scale_max=1.4",
              "environment.added_mass_min=-0.5", "environment.added_mass_max=4.0", "environment.added_mass_body=left_shin"]
EVERYTHING = RANDOMISED + ["environment.push_force=40", "environment.push_interval=5", "environment.push_duration=2", "environment.push_body=torso",
                           "environment.episode_length=4", "environment.reset_noise_scale=0.01", "training.normalize_observations=true",
                           "training.normalize_rewards=true"]
METRICS = tuple(METRIC_TYPES)


def test_engine_rollout_is_the_composition_of_the_public_stages(be):
    """Updates 0 and 1 of an engine with everything on, replayed by hand from what each started from: mppo_domain_fill once, then per step the engine's own
    action, mppo_push_fill + mppo_env_step_domain, mppo_env_time_limit, mppo_env_reset_domain over done (reset noise, event u T + 1 + t) and
    mppo_obs_norm_apply with the update's table - the engine's state, obs, reward, done, truncated and metrics regions bit for bit."""
    cfg = make_config(BASE, ENGINE + EVERYTHING)
    tr = be.trainer(cfg)
    cm, N, T, OP, A, O = tr.cm, tr.N, tr.T, tr.OP, tr.A, tr.O
    R = int(tr.dims.rec_dim)
    mass_body, push_body = list(cm.body_names).index("left_shin"), list(cm.body_names).index("torso")
    assert tr.domain.mass_body == mass_body and tr.push.body == push_body
    tr.reset()
    tr._sync()
    h, dims, _keep = be.model(cm)
    lib, s, p = be.lib, be.stream, be.ptr
    table = be.full((N, 4), np.nan)
    lib.domain_fill(C.byref(_dcfg(body=mass_body, seed=tr.seed)), N, p(table), s)
    be.sync()
    assert np.array_equal(_bits(be.host(table)), _bits(jaxrng.domain_params_philox(tr.seed, 0, N, **RANGES)))
    # the engine's reset: mppo_env_reset_domain, then the same over everyone under reset noise (event 0)
    st0, rr0, ob0 = be.zeros((N, R)), be.zeros((R,)), be.zeros((N, OP))
    m0 = {k: be.full((N,), 7, dt) for k, dt in METRIC_TYPES.items()}
    M0 = nat.EnvMetrics(**{k: p(v) for k, v in m0.items()})
    lib.env_reset_domain(h, N, p(st0), p(rr0), p(ob0), OP, None, None, C.byref(M0), None, p(table), mass_body, 0.0, 0, tr.seed, 0, None, None, 0, s)
    lib.env_reset_domain(h, N, p(st0), None, p(ob0), OP, None, None, None, None, p(table), mass_body, 0.01, 0, tr.seed, 0, None, None, 0, s)
    be.sync()
    assert np.array_equal(_bits(be.host(st0)), _bits(tr._to_host(tr.region("state", (N, R)))))
    assert np.array_equal(_bits(be.host(ob0)), _bits(tr._to_host(tr.region("obs", (T + 1, N, OP))[0])))
    assert np.array_equal(_bits(be.host(rr0)), _bits(tr._to_host(tr.region("reset_rec"))))
    pf = nat.PushCfg(body=push_body, interval=5, duration=2, rank=0, force=40.0, seed=tr.seed)
    lim = nat.TimeLimitCfg(length=4, stagger=1, rank=0, reserved=0, seed=tr.seed)
    ended = truncs = 0
    for u in range(2):
        start = tr._to_host(tr.region("state", (N, R))).copy()
        met0 = {k: tr._to_host(tr.region(k)).copy() for k in METRICS}
        norm = tr._to_host(tr.region("obs_norm_table")).copy()
        tr.update()
        tr._sync()
        eng = {k: tr._to_host(tr.region(k, shp)).copy() for k, shp in (("state", (N, R)), ("obs", (T + 1, N, OP)), ("reward", (T, N)), ("done", (T, N)),
                                                                       ("truncated", (T, N)), ("action", (T, N, A)))}
        eng_met = {k: tr._to_host(tr.region(k)).copy() for k in METRICS}
        state, reset_rec, ntab = be.arr(start), be.arr(tr._to_host(tr.region("reset_rec")).copy()), be.arr(norm)
        met = {k: be.arr(v) for k, v in met0.items()}
        Ms = nat.EnvMetrics(**{k: p(v) for k, v in met.items()})
        ctr = be.arr(np.array([u], np.int32))
        obs, rew, done, trunc, xfrc = be.zeros((N, OP)), be.zeros((N,)), be.zeros((N,), np.uint8), be.zeros((N,), np.uint8), be.zeros((N, 6))
        for t in range(T):
            act = be.arr(eng["action"][t])
            lib.push_fill(C.byref(pf), N, p(ctr), T, t, p(xfrc), s)
            lib.env_step_domain(h, N, 1, C.byref(tr.ecfg.reward), p(state), p(reset_rec), p(act), A, p(obs), OP, p(rew), p(done), C.byref(Ms), push_body, p(xfrc),
                                p(table), mass_body, s)
            lib.env_time_limit(h, N, C.byref(lim), p(state), p(reset_rec), p(obs), OP, p(done), p(trunc), C.byref(Ms), s)
            lib.env_reset_domain(h, N, p(state), None, p(obs), OP, None, None, None, p(done), p(table), mass_body, 0.01, 0, tr.seed, 0, None, None, u * T + 1 + t, s)
            lib.obs_norm_apply(N, O, p(obs), OP, p(ntab), OP, float(cfg.training.obs_norm_clip), None, s)
            be.sync()
            assert np.array_equal(_bits(be.host(obs)), _bits(eng["obs"][t + 1])), (u, t)
            assert np.array_equal(_bits(be.host(rew)), _bits(eng["reward"][t])), (u, t)
            assert np.array_equal(be.host(done), eng["done"][t]) and np.array_equal(be.host(trunc), eng["truncated"][t]), (u, t)
            ended, truncs = ended + int(be.host(done).sum()), truncs + int(be.host(trunc).sum())
        assert np.array_equal(_bits(be.host(state)), _bits(eng["state"])), u
        for k in METRICS:
            assert np.array_equal(_bits(be.host(met[k])), _bits(eng_met[k])), (u, k)
    assert truncs > 0 and ended >= truncs  # (the staggered limit of four steps cuts first episodes inside six: the restarts ran)
    lib.model_close(h)
    tr.close()


def _arena(tr, names=("params", "adam_m", "adam_v", "count", "state", "episode_returns", "episode_lengths", "returned_episode")):
    tr._sync()
    return {n: tr._to_host(tr.region(n)).copy() for n in names}


def _train(be, cfg, updates, before=None, **kw):
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


def test_default_ranges_are_an_engine_that_never_heard_of_the_randomisation(be):
    cfg = make_config(BASE, ENGINE)
    never, _ = _train(be, cfg, 2)
    ident = _dcfg(friction=(1, 1), actuator=(1, 1), mass=(0, 0), body=0)  # (off: not even the body is read)
    same, _ = _train(be, cfg, 2, before=lambda tr: be.lib.engine_set_domain(tr._engine, C.byref(ident)))
    null, _ = _train(be, cfg, 2, before=lambda tr: be.lib.engine_set_domain(tr._engine, None))
    rand, _ = _train(be, make_config(BASE, ENGINE + RANDOMISED), 2)
    for k in never:
        assert np.array_equal(_bits(never[k]), _bits(same[k])) and np.array_equal(_bits(never[k]), _bits(null[k])), k
    assert not np.array_equal(never["state"], rand["state"]) and np.isfinite(rand["params"]).all()
    tr = be.trainer(cfg)
    assert tr.domain is None  # (all six keys at their defaults: the trainer does not even make the call)
    tr.close()


def test_randomised_engine_checkpoints_and_resumes(be, tmp_path):
    cfg = make_config(BASE, ENGINE + EVERYTHING)
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
    assert int(tr._to_host(tr.region("done", (tr.T, tr.N))).sum()) > 0 or int(a4["episode_lengths"].min()) < 4 * tr.T  # (episodes ended on the way: resets crossed)
    tr.close()
    c = be.trainer(cfg)
    c.load_checkpoint(ck)
    for _ in range(2):
        c.update()
    c4 = _arena(c)
    c.close()
    for k in a4:
        assert np.array_equal(_bits(a4[k]), _bits(c4[k])), k
    if be.name == "hip":  # a replayed graph computes what eager launches compute
        e3, graph = _train(be, cfg, 3, use_graph=False)
        assert not graph
        for k in a3:
            assert np.array_equal(_bits(a3[k]), _bits(e3[k])), k


def test_set_domain_call_order_and_refusals(be):
    tr = be.trainer(make_config(BASE, ENGINE))
    f = be.lib._fn["mppo_engine_set_domain"]
    nb = tr.cm.nbody
    light = int(np.argmin(np.asarray(tr.cm.t["body_mass"])[1:])) + 1
    too_much = -float(tr.cm.t["body_mass"][light])
    for bad, word in ((_dcfg(body=0), "mass_body"), (_dcfg(body=nb), "mass_body"), (_dcfg(friction=(0.9, 0.5)), "friction_min"), (_dcfg(actuator=(2.0, 1.0)), "actuator_min"),
                      (_dcfg(mass=(1.0, 0.5)), "mass_min"), (_dcfg(friction=(-0.5, 1.0)), "negative"), (_dcfg(actuator=(-0.5, 1.0)), "negative"),
                      (_dcfg(mass=(too_much, 0.0), body=light), "without mass"), (_dcfg(friction=(float("nan"), 1.0)), "friction_min")):
        assert f(tr._engine, C.byref(bad)) != 0 and word in be.lib.last_error(), (word, be.lib.last_error())
    be.lib.engine_set_domain(tr._engine, C.byref(_dcfg()))
    be.lib.engine_set_domain(tr._engine, C.byref(_dcfg(rank=300, seed=1)))  # (rank and seed of the configuration are not read: the engine's are used)
    be.lib.engine_set_domain(tr._engine, None)
    tr.reset()
    assert f(tr._engine, C.byref(_dcfg())) == -4 and "mppo_engine_reset has run" in be.lib.last_error()  # MPPO_ESTATE
    tr.lib.engine_prepare(tr._engine, tr._stream_ptr)
    tr._sync()
    assert f(tr._engine, C.byref(_dcfg())) == -4
    assert "mppo_engine_set_domain" in be.lib.last_error() and "prepared" in be.lib.last_error()
    with pytest.raises(nat.NativeError):
        be.lib.engine_set_domain(tr._engine, C.byref(_dcfg()))
    tr.close()


# ---- 7: the evaluator and the host surface ----------------------------------------------------------------------------------------------------------------

EN, EK, ER, EH, EL = 20, 10, 3, 64, 4


def _eval_setup(be):
    from minppo_amd.train import init_flat_params

    cm = _cm("pro")
    h, dims, keep = be.model(cm)
    net = nat.Net(dims.obs_dim, dims.obs_pad, dims.nu, EH, 1, 0, 2)
    return cm, h, dims, keep, net, init_flat_params(3, dims.obs_dim, dims.nu, EH)


def _ecfg(noise=0.0):
    from minppo_amd.train import reward_cfg

    return nat.EvalCfg(N=EN, K=EK, n_frames=1, deterministic=1, record_envs=ER, reset_noise_scale=noise, seed=SEED, reward=reward_cfg(make_config(BASE)))


def _evaluate(be, domain, entry="domain", noise=0.0):
    cm, h, dims, keep, net, params = _eval_setup(be)
    e = _ecfg(noise)
    need = (be.lib.eval_domain_ws_bytes if entry == "domain" else be.lib.eval_limit_ws_bytes)(h, C.byref(net), C.byref(e))
    ws = be.full((need,), 0xA5, np.uint8)
    res = be.full(((C.sizeof(nat.EvalResultRaw) + C.sizeof(nat.EvalLimitResultRaw)) // 8,), -1, np.int64)
    traj = be.full((EK + 1, ER, cm.nq + cm.nv + dims.nu + 2), np.nan)
    p_dev = be.arr(params)
    extra = be.ptr(res) + C.sizeof(nat.EvalResultRaw)
    if entry == "domain":
        be.lib.evaluate_domain(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), need, None, 0.0, None, EL, C.byref(domain) if domain is not None else None,
                               be.ptr(res), extra, be.ptr(traj), be.stream)
    else:
        be.lib.evaluate_limit(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), need, None, 0.0, None, EL, be.ptr(res), extra, be.ptr(traj), be.stream)
    be.sync()
    out = (be.host(res).tobytes(), be.host(traj).copy())
    be.lib.model_close(h)
    return out


def _by_hand(be, domain, noise=0.0):
    """The documented sequence of mppo_evaluate_domain (episode length EL, no pushes, no table) written out with the library's entry points."""
    cm, h, dims, keep, net, params = _eval_setup(be)
    e = _ecfg(noise)
    lib, s, p = be.lib, be.stream, be.ptr
    OP, RD, A, nqv = dims.obs_pad, dims.rec_dim, dims.nu, cm.nq + cm.nv
    W = nqv + A + 2
    state, rec, obs = be.zeros((EN, RD)), be.zeros((RD,)), be.zeros((EN, OP))
    rew, done, trunc = be.zeros((EN,)), be.zeros((EN,), np.uint8), be.zeros((EN,), np.uint8)
    met = {k: be.full((EN,), 3, t) for k, t in METRIC_TYPES.items()}
    Ms = nat.EnvMetrics(**{k: p(v) for k, v in met.items()})
    p_dev = be.arr(params)
    act, logp, val, noise_buf = be.zeros((EN, A)), be.zeros((EN,)), be.zeros((EN,)), be.zeros((EN, A))
    wsb = lib.policy_ws_bytes(C.byref(net), EN)
    ws = be.zeros((wsb,), np.uint8)
    acc, lacc = be.full((nat.EVAL_ACC_SLOTS * EN,), -1, np.int64), be.full((2 * EN,), -1, np.int64)
    res = be.full(((C.sizeof(nat.EvalResultRaw) + C.sizeof(nat.EvalLimitResultRaw)) // 8,), -1, np.int64)
    d = nat.DomainCfg.from_buffer_copy(domain)
    d.rank, d.seed = 0, e.seed
    table = be.full((EN, 4), np.nan)
    lim = nat.TimeLimitCfg(length=EL, stagger=0, rank=0, reserved=0, seed=e.seed)
    lib.domain_fill(C.byref(d), EN, p(table), s)
    lib.env_reset_domain(h, EN, p(state), p(rec), p(obs), OP, p(rew), p(done), C.byref(Ms), None, p(table), d.mass_body, 0.0, 0, e.seed, 0, None, None, 0, s)
    if noise > 0:
        lib.env_reset_domain(h, EN, p(state), None, p(obs), OP, None, None, None, None, p(table), d.mass_body, noise, 0, e.seed, 0, None, None, 0, s)
    be.sync()
    frame0 = np.zeros((ER, W), f32)
    frame0[:, :nqv] = be.host(state)[:ER, :nqv]
    rows = [frame0]
    for t in range(EK):
        lib.policy_forward(C.byref(net), p(p_dev), EN, p(obs), OP, p(noise_buf), p(act), p(logp), p(val), 0, p(ws), wsb, s)
        lib.env_step_domain(h, EN, e.n_frames, C.byref(e.reward), p(state), p(rec), p(act), A, p(obs), OP, p(rew), p(done), C.byref(Ms), 0, None, p(table), d.mass_body, s)
        lib.env_time_limit(h, EN, C.byref(lim), p(state), p(rec), p(obs), OP, p(done), p(trunc), C.byref(Ms), s)
        lib.env_reset_domain(h, EN, p(state), None, p(obs), OP, None, None, None, p(done), p(table), d.mass_body, noise, 0, e.seed, 0, None, None, t + 1, s)
        row = be.zeros((ER, W))
        lib.eval_accumulate(EN, int(t == 0), p(rew), p(done), C.byref(Ms), p(acc), p(state), RD, nqv, p(act), A, A, ER, p(row), s)
        lib.eval_limit_count(EN, int(t == 0), p(done), p(trunc), p(lacc), s)
        be.sync()
        rows.append(be.host(row).copy())
    lib.eval_limit_reduce(EN, p(lacc), p(res) + C.sizeof(nat.EvalResultRaw), s)
    lib.eval_reduce(EN, EK, p(acc), p(res), s)
    be.sync()
    out = (be.host(res).tobytes(), np.stack(rows), be.host(table).copy())
    lib.model_close(h)
    return out


@pytest.mark.parametrize("noise", [0.0, 0.01])
def test_evaluate_domain_is_its_composition(be, noise):
    dom = _dcfg(body=_leaf(_cm("pro")), rank=3, seed=999)  # (rank and seed of the configuration are not read)
    raw, traj = _evaluate(be, dom, noise=noise)
    raw_h, traj_h, table = _by_hand(be, dom, noise)
    assert np.array_equal(_bits(table), _bits(jaxrng.domain_params_philox(SEED, 0, EN, **RANGES)))
    assert not np.isnan(traj).any() and traj[..., -1].any()  # (the limit of four steps cut episodes: the restarts ran)
    assert np.array_equal(_bits(traj), _bits(traj_h))
    assert raw == raw_h
    # domain = NULL and every range at its identity: mppo_evaluate_limit
    plain = _evaluate(be, None, entry="limit", noise=noise)
    for off in (None, _dcfg(friction=(1, 1), actuator=(1, 1), mass=(0, 0), body=0)):
        got = _evaluate(be, off, noise=noise)
        assert got[0] == plain[0] and np.array_equal(_bits(got[1]), _bits(plain[1]))
    assert not np.array_equal(traj, plain[1])


def test_evaluate_domain_refuses_bad_configurations(be):
    cm, h, dims, keep, net, params = _eval_setup(be)
    e = _ecfg()
    need = be.lib.eval_domain_ws_bytes(h, C.byref(net), C.byref(e))
    ws, res, p_dev = be.zeros((need,), np.uint8), be.zeros((16,), np.int64), be.arr(params)
    traj = be.zeros((EK + 1, ER, cm.nq + cm.nv + dims.nu + 2))
    f = be.lib._fn["mppo_evaluate_domain"]
    light = int(np.argmin(np.asarray(cm.t["body_mass"])[1:])) + 1
    for bad, word in ((_dcfg(body=0), "mass_body"), (_dcfg(body=cm.nbody), "mass_body"), (_dcfg(friction=(2.0, 1.0)), "friction_min"), (_dcfg(actuator=(-1.0, 1.0)), "negative"),
                      (_dcfg(mass=(-float(cm.t["body_mass"][light]), 1.0), body=light), "without mass")):
        assert f(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), need, 0, 0.0, None, 0, C.byref(bad), be.ptr(res), be.ptr(res) + 96, be.ptr(traj), be.stream) != 0
        assert word in be.lib.last_error(), (word, be.lib.last_error())
    small = be.lib.eval_limit_ws_bytes(h, C.byref(net), C.byref(e))
    assert small < need
    assert f(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), small, 0, 0.0, None, 0, C.byref(_dcfg()), be.ptr(res), be.ptr(res) + 96, be.ptr(traj), be.stream) != 0
    assert "mppo_eval_domain_ws_bytes" in be.lib.last_error()
    be.lib.model_close(h)


def test_python_evaluate_goes_through_the_randomised_entry_point(be):
    from minppo_amd.evaluate import evaluate, result_from_struct
    from minppo_amd.train import init_flat_params

    cm = _cm("pro")
    raw, traj = _evaluate(be, _dcfg(body=list(cm.body_names).index("left_shin")))
    cfg = make_config(BASE, [f"model.hidden_size={EH}", f"training.seed={SEED}", f"evaluation.num_envs={EN}", f"evaluation.num_steps={EK}", f"evaluation.record_envs={ER}",
                             f"environment.episode_length={EL}"] + RANDOMISED)
    flat = init_flat_params(3, cm.obs_size(True), cm.nu, EH)
    device = {} if be.name == "emu" else {"device": "cuda:0"}
    got = evaluate(cfg, flat, lib=be.lib, xp=be.xp, **device)
    want = result_from_struct(nat.EvalResultRaw.from_buffer_copy(raw[:C.sizeof(nat.EvalResultRaw)]))
    for k in ("episodes", "mean_return", "mean_length", "mean_reward", "steps"):
        assert got.stats()[k] == want.stats()[k], k
    assert np.array_equal(_bits(got.trajectory["qpos"]), _bits(traj[..., :cm.nq]))
    echo = {"friction_scale_min": 0.3, "friction_scale_max": 1.7, "actuator_scale_min": 0.6, "actuator_scale_max": 1.4, "added_mass_min": -0.5, "added_mass_max": 4.0}
    assert {k: got.stats()[k] for k in echo} == echo
    assert "friction_scale_min" not in evaluate(make_config(BASE, [f"model.hidden_size={EH}", "evaluation.num_envs=4", "evaluation.num_steps=2"]), flat, lib=be.lib,
                                                xp=be.xp, **device).stats()


def test_config_keys_defaults_and_refusals():
    env = make_config(BASE).environment
    assert (env.friction_scale_min, env.friction_scale_max, env.actuator_scale_min, env.actuator_scale_max, env.added_mass_min, env.added_mass_max,
            env.added_mass_body) == (1.0, 1.0, 1.0, 1.0, 0.0, 0.0, "")
    got = make_config(BASE, RANDOMISED).environment
    assert (got.friction_scale_min, got.friction_scale_max, got.actuator_scale_min, got.actuator_scale_max, got.added_mass_min, got.added_mass_max,
            got.added_mass_body) == (0.3, 1.7, 0.6, 1.4, -0.5, 4.0, "left_shin")
    for what in ("friction_scale", "actuator_scale", "added_mass"):
        with pytest.raises(ValueError, match=what + "_min"):
            make_config(BASE, [f"environment.{what}_min=2.0", f"environment.{what}_max=1.5"])
    for what in ("friction_scale", "actuator_scale"):
        with pytest.raises(ValueError, match="negative"):
            make_config(BASE, [f"environment.{what}_min=-0.5"])
    make_config(BASE, ["environment.added_mass_min=-0.5"])  # (a payload may be negative: a lighter trunk)


def test_unknown_added_mass_body_names_the_bodies():
    from minppo_amd.train import domain_body_id, domain_cfg, domain_on, resolve_model

    with pytest.raises(ValueError, match=r"added_mass_body.*nose.*torso.*left_shin"):
        resolve_model(make_config(BASE, ["environment.added_mass_max=2", "environment.added_mass_body=nose"]))
    with pytest.raises(ValueError, match="added_mass_body"):
        resolve_model(make_config(BASE, ["environment.friction_scale_min=0.5", "environment.added_mass_body=world"]))
    cm = resolve_model(make_config(BASE, ["environment.added_mass_body=nose"]))  # (every range at its default: the name is not read)
    assert not domain_on(make_config(BASE)) and domain_cfg(make_config(BASE), cm) is None
    d = domain_cfg(make_config(BASE, RANDOMISED), cm, seed=9, rank=2)
    assert (d.mass_body, d.rank, d.seed) == (list(cm.body_names).index("left_shin"), 2, 9)
    assert [round(x, 6) for x in (d.friction_min, d.friction_max, d.actuator_min, d.actuator_max, d.mass_min, d.mass_max)] == [0.3, 1.7, 0.6, 1.4, -0.5, 4.0]
    assert domain_cfg(make_config(BASE, ["environment.added_mass_max=1"]), cm).mass_body == 1
    named = make_config(BASE, ["environment.added_mass_body=left_shin"])
    assert domain_body_id(named, cm) == 1 and domain_body_id(named, cm, always=True) == list(cm.body_names).index("left_shin")


@pytest.mark.gpu
def test_humanoid_env_takes_a_table_and_draws_one():
    import torch

    from minppo_amd.env import HumanoidEnv

    N = 5
    env = HumanoidEnv(make_config(BASE, RANDOMISED + [f"training.seed={SEED}"]))
    cm = env.cm
    body = list(cm.body_names).index("left_shin")
    want = jaxrng.domain_params_philox(SEED, 0, N, **RANGES)
    assert np.array_equal(_bits(env.domain_params(N).cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(env.domain_params(N, seed=77).cpu().numpy()), _bits(jaxrng.domain_params_philox(77, 0, N, **RANGES)))
    act = 0.3 * torch.ones(N, env.action_size, device=env.device)
    es = env.reset(num_envs=N)  # the drawn table
    assert np.array_equal(_bits(env._domain.cpu().numpy()), _bits(want))
    e1 = env.step(es, act)
    # the C calls
    lib, d, s = env.lib, env.dims, torch.cuda.current_stream(env.device).cuda_stream
    tab = torch.from_numpy(want).to(env.device)
    state, rr = torch.empty(N, d.rec_dim, device=env.device), torch.empty(d.rec_dim, device=env.device)
    obs, rew, done = torch.empty(N, d.obs_pad, device=env.device), torch.empty(N, device=env.device), torch.empty(N, dtype=torch.uint8, device=env.device)
    lib.env_reset_domain(env._model, N, state.data_ptr(), rr.data_ptr(), obs.data_ptr(), d.obs_pad, rew.data_ptr(), done.data_ptr(), None, None, tab.data_ptr(), body, 0.0,
                         0, 0, 0, None, None, 0, s)
    torch.cuda.synchronize()
    assert torch.equal(es.pipeline_state, state)
    lib.env_step_domain(env._model, N, 1, C.byref(env._rc), state.data_ptr(), rr.data_ptr(), act.data_ptr(), env.action_size, obs.data_ptr(), d.obs_pad, rew.data_ptr(),
                        done.data_ptr(), None, 0, None, tab.data_ptr(), body, s)
    lib.env_reset_domain(env._model, N, state.data_ptr(), None, obs.data_ptr(), d.obs_pad, None, None, None, done.data_ptr(), tab.data_ptr(), body, 0.0, 0, 0, 0, None, None,
                         0, s)
    torch.cuda.synchronize()
    assert torch.equal(e1.pipeline_state, state) and torch.equal(e1.reward, rew)
    # a given table; the identity table is the plain environment
    rows = torch.from_numpy(ROWS[:N].copy())
    g0 = env.reset(num_envs=N, domain=rows)
    assert not torch.equal(g0.pipeline_state, es.pipeline_state)
    g1 = env.step(g0, act)
    ident = torch.tensor([[1.0, 1.0, 0.0, 0.0]]).repeat(N, 1)
    i1 = env.step(env.reset(num_envs=N, domain=ident), act)
    for bad in (torch.zeros(N, 3), torch.zeros(N + 1, 4), torch.zeros(4)):
        with pytest.raises(ValueError, match="domain"):
            env.reset(num_envs=N, domain=bad)
    env.reset(num_envs=N + 1)
    with pytest.raises(ValueError, match="reset"):
        env.step(es, act)
    env.close()
    plain = HumanoidEnv(make_config(BASE))
    with pytest.raises(ValueError, match="default"):
        plain.domain_params(N)
    p1 = plain.step(plain.reset(num_envs=N), act)
    assert torch.equal(p1.pipeline_state, i1.pipeline_state) and not torch.equal(p1.pipeline_state, g1.pipeline_state)
    plain.close()
    with pytest.raises(ValueError, match=r"added_mass_body.*nose.*left_shin"):
        HumanoidEnv(make_config(BASE, ["environment.added_mass_body=nose"]))


@pytest.mark.gpu
def test_train_and_evaluate_at_a_fixed_friction_from_the_command_line(tmp_path):
    model = str(tmp_path / "model.pkl")
    small = ["training.num_envs=64", "training.num_minibatches=2", "model.hidden_size=64"]
    p = subprocess.run([sys.executable, "-m", "minppo_amd.cli", "train", "stompy_pro", *small, *RANDOMISED, "training.total_timesteps=1920", f"training.model_save_path={model}"],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert p.returncode == 0 and Path(model).exists(), p.stderr[-2000:]
    p = subprocess.run([sys.executable, "-m", "minppo_amd.cli", "evaluate", "stompy_pro", *small, "evaluation.num_envs=20", "evaluation.num_steps=8",
                        "environment.friction_scale_min=0.3", "environment.friction_scale_max=0.3", f"inference.model_path={model}"], capture_output=True, text=True,
                       cwd=str(ROOT), timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1
    out = json.loads(line[0])
    assert set(out) == {"episodes", "mean_return", "std_return", "min_return", "max_return", "mean_length", "min_length", "max_length", "survivors", "survivor_mean_return",
                        "mean_reward", "steps", "friction_scale_min", "friction_scale_max", "actuator_scale_min", "actuator_scale_max", "added_mass_min", "added_mass_max"}
    assert (out["friction_scale_min"], out["friction_scale_max"], out["actuator_scale_min"], out["actuator_scale_max"], out["added_mass_min"], out["added_mass_max"]) == (
        0.3, 0.3, 1.0, 1.0, 0.0, 0.0)
