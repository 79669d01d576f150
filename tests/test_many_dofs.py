"""Robots of more than 64 dofs (up to model.MAX_DOFS = 128): the environment kernel's dof sets - body_ancdof_mask per body, dof_velmask per
dof, the per-contact-slot jmask - carry a second 64-bit word (dofs 64 .. 127) behind the first.  A 64-bit shift on gfx950 uses the low six
bits of its amount, so a dof-set site that still reads one word turns dof 70 into dof 6: the known-answer test below is built to see that.

The fixture, tests/golden/many_dofs/hands_humanoid.xml (tests/golden/many_dofs/make_hands_humanoid.py): a humanoid with two five-finger hands, 77 dofs, the
arms and hands declared before the legs - every leg dof, leg limit, leg actuator and foot contact row sits at dof index 65 .. 76.  Its
fingers are coupled by joint equalities (mimic joints): the float64 oracle (oracle/physics_oracle.py) puts MJX's equality rows first in
the constraint; variants without the equalities are compared at test_forward_matches_oracle's tolerances."""

import ctypes as C
import os
from pathlib import Path

import numpy as np
import pytest

from minppo_amd import _native as nat
from minppo_amd import model as M
from minppo_amd.mjcf import load_mjcf
from minppo_amd.model import JNT_FREE, JNT_HINGE, JNT_SLIDE, MAX_DOFS, compile_model, load_model
from oracle.env_oracle import EnvOracle, RewardCfg
from oracle.physics_oracle import Physics, PhysState
from physics_harness import (SMOOTH_TOL, assert_bit_equal, check_against_oracle, cost, euler_acc, pack, probe, probe_and_steps, random_states,
                             startup_kernel_equals_runtime_sized, walking_states)

f32, f64 = np.float32, np.float64
HANDS = str(Path(__file__).parent / "golden" / "many_dofs" / "hands_humanoid.xml")  # (a directory of its own: tests/golden/*.xml are the
# models whose tables tests/golden/table_sha256.json pins)


def _spec(equalities=True, legs_first=False):
    spec = load_mjcf(HANDS)
    if not equalities:
        spec.equalities = []
    if legs_first:  # the legs' subtrees right behind the pelvis: their dofs become 6 .. 17, the hands' reach 76
        legs = [b for b in spec.bodies if b.name.split("_", 1)[-1] in ("thigh", "shin", "foot")]
        rest = [b for b in spec.bodies if b not in legs]
        spec.bodies = rest[:1] + legs + rest[1:]
    return spec


def _sets(t, nbody, nv):
    """Both dof-set tables as Python integers of up to 128 bits (word 0 | word 1 << 64)."""
    def words(name, n):
        w = np.asarray(t[name], np.int32).view(np.uint64)
        assert w.size == (2 if nv > 64 else 1) * n, name
        return [int(w[i]) | (int(w[n + i]) << 64 if nv > 64 else 0) for i in range(n)]
    return words("body_ancdof_mask", nbody), words("dof_velmask", nv)


def _sets_from_tree(cm):
    """The same sets from the kinematic tree alone: the dofs of a body and its ancestors; for cdof_dot of dof d, the dofs numbered before the
    first dof of d's group (the joint; a free joint's translation, or its rotation) whose body is d's body or one of its ancestors."""
    t = cm.t
    par, dof_body, jnt = t["body_parent"], t["dof_bodyid"], t["dof_jntid"]

    def anc_or_self(b):
        out = set()
        while b > 0:
            out.add(int(b))
            b = par[b]
        return out

    anc = [sum(1 << d for d in range(cm.nv) if int(dof_body[d]) in anc_or_self(b)) if b else 0 for b in range(cm.nbody)]
    vel = []
    for d in range(cm.nv):
        j = int(jnt[d])
        da = int(t["jnt_dofadr"][j])
        first = (da if d < da + 3 else da + 3) if int(t["jnt_type"][j]) == JNT_FREE else d
        bodies = anc_or_self(dof_body[d])
        vel.append(sum(1 << e for e in range(first) if int(dof_body[e]) in bodies))
    return anc, vel


def _dof(cm, joint):
    return int(cm.t["jnt_dofadr"][cm.joint_names.index(joint)])


def _body(cm, name):
    return cm.body_names.index(name)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the compiler
# ---------------------------------------------------------------------------------------------------------------------------------------


def test_fixture_compiles_with_two_word_dof_sets():
    cm = load_model(HANDS)
    assert 64 < cm.nv <= MAX_DOFS and cm.nq == cm.nv + 1 and cm.nu <= 63 and 0 < cm.neq <= M.MAX_EQ_ROWS and cm.nbody <= 64
    t = cm.t
    # the legs are declared last: their dofs, limits, actuators and the feet's contact slots all sit beyond dof 63
    leg = [_dof(cm, f"{s}_{j}") for s in "lr" for j in ("hip_z", "hip_x", "hip_y", "knee", "ankle_y", "ankle_x")]
    assert min(leg) >= 64 and max(leg) == cm.nv - 1
    lim_dofs = [int(t["jnt_dofadr"][j]) for j in t["lim_jntid"]]
    assert set(leg) <= set(lim_dofs) and set(leg) <= {int(d) for d in t["act_dofid"]}
    feet = {_body(cm, "l_foot"), _body(cm, "r_foot")}
    assert sum(int(b) in feet for b in t["con_bodyid"]) == 8  # (two boxes against the plane: four corner slots each)
    anc, vel = _sets(t, cm.nbody, cm.nv)
    anc_ref, vel_ref = _sets_from_tree(cm)
    assert anc == anc_ref and vel == vel_ref
    assert any(m >> 64 for m in anc) and any(m >> 64 for m in vel)
    # a body that only dofs >= 64 move: its word 0 holds the free root alone
    assert anc[_body(cm, "r_foot")] & ((1 << 64) - 1) == (1 << 6) - 1


def test_the_dof_cap():
    def chain(ndof):
        bodies, left, k, parent = [M.BodySpec("root", "world", joints=[M.JointSpec("free", JNT_FREE)])], ndof - 6, 0, "root"
        while left > 0:
            n = min(3, left)
            bodies.append(M.BodySpec(f"b{k}", parent, pos=(0.0, 0.0, -0.05), mass=0.1, inertia=(1e-3, 1e-3, 1e-3),
                                     joints=[M.JointSpec(f"j{k}_{i}", JNT_HINGE, axis=((1, 0, 0), (0, 1, 0), (0, 0, 1))[i]) for i in range(n)]))
            parent, k, left = f"b{k}", k + 1, left - n
        return M.ModelSpec(f"chain_{ndof}", bodies, [])

    cm = compile_model(chain(MAX_DOFS))
    assert cm.nv == 128 and cm.nq == 129
    anc, vel = _sets(cm.t, cm.nbody, cm.nv)
    assert (anc, vel) == _sets_from_tree(cm) and anc[-1] == (1 << 128) - 1
    with pytest.raises(ValueError, match=r"at most 128 bodies .* and 128 dofs .* 129 dofs"):
        compile_model(chain(MAX_DOFS + 1))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the largest robots get a layout
# ---------------------------------------------------------------------------------------------------------------------------------------


def _largest_robot():
    """128 dofs, 124 bodies, 123 contact slots (a sphere on every link), 122 limited hinges: 614 constraint rows.  Its contact Jacobian alone
    would take 254 KB of LDS per environment and M another 66 KB: both go to global memory (model_view.h spill_for)."""
    bodies = [M.BodySpec("root", "world", mass=2.0, inertia=(0.02, 0.02, 0.02), joints=[M.JointSpec("free", JNT_FREE)],
                         geoms=[M.GeomSpec(M.GEOM_SPHERE, (0.05,))])]
    rng = np.random.default_rng(5)
    for k in range(122):
        parent = "root" if k < 4 else f"b{int(rng.integers(max(0, k - 6), k))}"
        bodies.append(M.BodySpec(f"b{k}", parent, pos=tuple(0.06 * rng.normal(size=3)), mass=0.2, inertia=(2e-4, 2e-4, 2e-4),
                                 joints=[M.JointSpec(f"j{k}", JNT_HINGE, axis=tuple(rng.normal(size=3)), range=(-0.5, 0.5), damping=0.2, armature=0.01)],
                                 geoms=[M.GeomSpec(M.GEOM_SPHERE, (0.02,))]))
    return M.ModelSpec("largest", bodies, [M.ActuatorSpec(f"j{k}", kp=2.0) for k in (0, 60, 121)], free_root_z=0.3)


def test_128_dof_robots_get_a_layout_within_lds(be):
    for cm in (compile_model(_largest_robot()), load_model(HANDS)):
        h, dims, _keep = be.model(cm)
        nb = C.c_size_t(0)
        be.lib.model_scratch_bytes(h, 4096, C.byref(nb))
        assert 0 < dims.lds_bytes <= 160 * 1024 and nb.value > 0, (cm.name, dims.lds_bytes, nb.value)
        be.lib.model_close(h)
    cm = compile_model(_largest_robot())
    assert cm.nv == 128 and cm.nefc == 614
    _forward_vs_oracle(be, cm, N=2, seed=3, solver=False)


# ---------------------------------------------------------------------------------------------------------------------------------------
# known answer: the second word, and nothing of it aliased into the first
# ---------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("spill", [None, "0"])
def test_a_dof_beyond_64_moves_its_subtree_only(be, monkeypatch, spill):
    """Every velocity zero but that of the right ankle (dof d = 75; d - 64 = 11 is the left shoulder).  The root sunk 0.8 m: the feet and
    fingertips are in contact.  cvel is non-zero exactly on the right foot; column k of a contact's Jacobian rows is zero whenever dof
    k does not move the contact's body - so column d is exactly zero on a left fingertip (which dof d - 64 does move: a one-word test of d
    reads it) and on the left foot (which neither moves).  Also with the Jacobian in LDS (MPPO_ENV_SPILL=0, the run-time-sized kernel)."""
    if spill is None:
        monkeypatch.delenv("MPPO_ENV_SPILL", raising=False)
    else:
        monkeypatch.setenv("MPPO_ENV_SPILL", spill)
    cm = load_model(HANDS)
    t = cm.t
    d = _dof(cm, "r_ankle_y")
    assert d >= 64 and d - 64 == _dof(cm, "l_shoulder_y")
    h, dims, _keep = be.model(cm)
    assert dims.lds_bytes <= 160 * 1024
    N = 2
    qpos = np.tile(np.asarray(t["qpos0"], f64), (N, 1))
    qpos[:, 2] -= 0.8
    qpos[1, int(t["jnt_qposadr"][cm.joint_names.index("r_knee")])] = 0.7  # (a second pose: the joint axes move)
    qvel = np.zeros((N, cm.nv))
    qvel[:, d] = 1.5
    got = probe(be, h, cm, qpos.astype(f32), qvel.astype(f32), np.zeros((N, cm.nu), f32), np.zeros((N, cm.nv), f32))
    be.lib.model_close(h)
    anc, _ = _sets(t, cm.nbody, cm.nv)
    moved = np.array([(anc[b] >> d) & 1 for b in range(cm.nbody)], bool)
    assert moved.sum() == 1 and moved[_body(cm, "r_foot")]
    cvel = got["cvel"].reshape(N, cm.nbody, 6)
    assert (np.abs(cvel[:, moved]).max(-1) > 0.1).all() and (cvel[:, ~moved] == 0).all()
    J = got["efc_J"].reshape(N, cm.nefc, cm.nv)
    D = got["efc_D"].reshape(N, cm.nefc)
    r0 = cm.neq + cm.nlimit
    tips = {_body(cm, f"l_{f}_dist") for f in ("index", "middle", "ring", "little", "thumb")}
    seen = {"tip": 0, "lfoot": 0, "rfoot": 0}
    for n in range(N):
        for c, b in enumerate(int(x) for x in t["con_bodyid"]):
            Jc = J[n, r0 + 4 * c:r0 + 4 * c + 4]
            if not (D[n, r0 + 4 * c:r0 + 4 * c + 4] > 0).all():  # (a box corner plane_convex picked twice: switched off, its rows are zeros)
                assert (Jc == 0).all(), (n, c)
                continue
            nz = np.abs(Jc).max(0) > 0  # which columns the slot's rows touch
            want = np.array([(anc[b] >> k) & 1 for k in range(cm.nv)], bool)
            assert not (nz & ~want).any(), (n, c, cm.body_names[b], np.argwhere(nz & ~want).tolist())
            assert nz[want].mean() > 0.8, (n, c, cm.body_names[b])  # (a dof whose axis runs through the contact point moves it by nothing)
            if b in tips:
                assert (Jc[:, d] == 0).all() and (Jc[:, d - 64] != 0).any()
                seen["tip"] += 1
            elif b == _body(cm, "l_foot"):
                assert (Jc[:, d] == 0).all() and (Jc[:, d - 64] == 0).all()
                seen["lfoot"] += 1
            elif b == _body(cm, "r_foot"):
                assert (Jc[:, d] != 0).any()
                seen["rfoot"] += 1
    assert seen["tip"] == 5 * N and seen["lfoot"] >= 2 * N and seen["rfoot"] >= 2 * N, seen


# ---------------------------------------------------------------------------------------------------------------------------------------
# forward pass against the float64 oracle / reference
# ---------------------------------------------------------------------------------------------------------------------------------------


def _forward_vs_oracle(be, cm, N, seed, solver=True, states=None):
    """The comparisons of tests/test_kernels_physics.py::test_forward_matches_oracle at its tolerances: tight before the solver, the solver through
    its cost and the Euler envelope."""
    h, dims, _keep = be.model(cm)
    assert dims.obs_dim == cm.obs_size() and dims.nefc == cm.nefc and dims.lds_bytes <= 160 * 1024
    qpos, qvel, ctrl, warm = states if states is not None else walking_states(cm, N, seed)
    q32 = [x.astype(f32) for x in (qpos, qvel, ctrl if cm.nu else np.zeros((N, 1)), warm)]
    ref = PhysState(qpos=q32[0].astype(f64), qvel=q32[1].astype(f64), ctrl=q32[2].astype(f64)[:, :cm.nu], qacc_warmstart=q32[3].astype(f64), time=np.zeros(N))
    Physics(cm.t).forward(ref)
    got = probe(be, h, cm, *q32)
    be.lib.model_close(h)
    tol = dict(qM=1e-5, qfrc_bias=1e-4, qfrc_passive=1e-5, qfrc_actuator=1e-5, qacc_smooth=2e-4, efc_J=1e-5, efc_D=5e-4, efc_aref=5e-4, cinert=1e-5,
               cvel=1e-4, xpos=1e-5)
    for k, t in tol.items():
        r = ref[k]
        if r.size:
            scale = np.abs(r).max() + 1e-6
            err = np.abs(got[k].reshape(r.shape) - r).max()
            assert err <= t * scale, (cm.name, k, err / scale)
    assert np.allclose(got["subtree_com1"], ref.subtree_com[:, 1, 0], atol=1e-5)
    if not solver:
        return
    c_got, c_ref, c_smooth = cost(ref, got["qacc"]), cost(ref, ref.qacc), cost(ref, ref.qacc_smooth)
    np.testing.assert_allclose(c_got, c_ref, rtol=5e-2, atol=1e-3)
    assert np.all(c_got <= c_smooth * (1 + 1e-5) + 1e-6) and np.all(got["niter"] <= 6)
    rel = np.abs(got["qacc"] - ref.qacc).max(1) / (np.abs(ref.qacc).max(1) + 1e-9)
    assert np.median(rel) <= 5e-3 and rel.max() <= 0.3, (cm.name, np.median(rel), rel.max())
    ref_e = euler_acc(cm, ref)
    rel_e = np.abs(got["qacc_euler"] - ref_e).max(1) / (np.abs(ref_e).max(1) + 1e-9)
    # (the fixture's fingers are light end bodies whose implicit damping h D exceeds their inertia, as on the export-style biped: measured on the
    # emulator, per-state 3e-3 .. 8.4e-2 (median 2.2e-2) as declared, 2e-4 .. 2.5e-2 legs first - and the float32 ORACLE on the same states
    # 0 .. 0.42 from float64: the solver's float32 envelope, not the kernel.  Bounds of test_forward_matches_oracle's export biped.)
    lim_med, lim_q90 = (5e-2, 0.7) if cm.name.startswith("hands_humanoid") else (5e-3, 0.3)
    assert np.median(rel_e) <= lim_med and np.quantile(rel_e, 0.9) <= lim_q90, (cm.name, np.median(rel_e), rel_e.max())


@pytest.mark.parametrize("legs_first", [False, True])
def test_forward_without_equalities_matches_the_oracle(be, legs_first):
    """The fixture with its mimic equalities taken out, as declared and with the legs first: oracle/physics_oracle.py, the tolerances of
    test_forward_matches_oracle."""
    cm = compile_model(_spec(equalities=False, legs_first=legs_first))
    assert cm.nv == 77 and cm.neq == 0
    if legs_first:
        assert max(_dof(cm, f"{s}_{j}") for s in "lr" for j in ("hip_z", "ankle_x")) < 64 and _dof(cm, "r_thumb_dip") == cm.nv - 1
    _forward_vs_oracle(be, cm, N=6, seed=5)


@pytest.mark.parametrize("legs_first", [False, True])
def test_fixture_follows_the_equality_reference(be, legs_first):
    """The fixture itself (mimic rows first in the constraint) at the tolerances test_equality.py holds its fixtures to."""
    cm = compile_model(_spec(legs_first=legs_first))
    assert cm.neq == 10
    for s in range(2):
        # (the solver's cost on the median, at most 0.3 away in single states - the bound of test_equality.py's random robots: measured on the
        # emulator, one of the six legs-first states of seed 11 ends 0.26 from the float64 cost, the others within 2e-3)
        check_against_oracle(be, cm, walking_states(cm, 6, 10 + s), f"hands/{legs_first}/{s}", SMOOTH_TOL, dict(efc_J=1e-5, efc_D=5e-4, efc_aref=5e-4), min_good=3,
                             strict_cost=False)


# ---------------------------------------------------------------------------------------------------------------------------------------
# random robots of 65 .. 128 dofs
# ---------------------------------------------------------------------------------------------------------------------------------------


def random_many_dof_model(seed: int) -> M.ModelSpec:
    """A free root and a forest of hinge / slide joints (one or two per body; now and then a tree hinged on the world) up to a random dof count
    in 65 .. 128; spheres and capsules against the ground, a few more that meet each other (pair contacts); limits and actuators on the first
    and the last joint, and on others at random."""
    rng = np.random.default_rng(9000 + seed)
    target = int(rng.integers(65, MAX_DOFS + 1))

    def unit():
        v = rng.normal(size=3)
        return tuple(v / np.linalg.norm(v))

    bodies = [M.BodySpec("b0", "world", mass=3.0, inertia=(0.05, 0.05, 0.05), joints=[M.JointSpec("root", JNT_FREE)],
                         geoms=[M.GeomSpec(M.GEOM_SPHERE, (0.08,))])]
    acts, nv, joints = [], 6, []
    while nv < target and len(bodies) < 120:
        k = len(bodies)
        nj = 2 if (rng.random() < 0.3 and nv + 2 <= target) or target - nv > 2 * (124 - k) else 1
        parent = "world" if rng.random() < 0.04 else f"b{int(rng.integers(max(0, k - 8), k))}"
        js = []
        for i in range(nj):
            jt = JNT_HINGE if rng.random() < 0.8 else JNT_SLIDE
            js.append(M.JointSpec(f"b{k}_j{i}", jt, pos=tuple(0.03 * rng.normal(size=3)), axis=unit(), range=(-0.6, 0.6) if rng.random() < 0.5 else None,
                                  damping=float(rng.uniform(0.05, 1.0)), armature=float(rng.uniform(0.005, 0.03))))
        u = rng.random()
        geoms = [M.GeomSpec(M.GEOM_SPHERE, (float(rng.uniform(0.02, 0.05)),), pos=tuple(0.03 * rng.normal(size=3)))] if u < 0.2 else \
                [M.GeomSpec(M.GEOM_CAPSULE, (0.02, 0.04), quat=(0.7071, 0.7071, 0.0, 0.0))] if u < 0.28 else \
                [M.GeomSpec(M.GEOM_SPHERE, (0.04,), contype=2, conaffinity=2)] if u < 0.33 else []
        pos = (float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-0.5, 0.5)), 0.3) if parent == "world" else tuple(0.08 * rng.normal(size=3))
        bodies.append(M.BodySpec(f"b{k}", parent, pos=pos, mass=float(rng.uniform(0.1, 1.0)), inertia=(2e-3, 2e-3, 1e-3), joints=js, geoms=geoms))
        joints += js
        nv += nj
    for j in (joints[0], joints[-1]):
        j.range = (-0.4, 0.4)
    for i, j in enumerate(joints):
        if i in (0, len(joints) - 1) or rng.random() < 0.3:
            acts.append(M.ActuatorSpec(j.name, kp=float(rng.uniform(2, 20)), ctrlrange=(-1.0, 1.0)))
    return M.ModelSpec(f"many_dof_{seed}", bodies, acts, free_root_z=0.25)


MANY_DOF_SEEDS = list(range(int(os.environ.get("MPPO_FUZZ_MANY_DOF_ROBOTS", "4"))))


@pytest.mark.parametrize("seed", MANY_DOF_SEEDS)
def test_kernel_follows_the_oracle_on_a_random_many_dof_robot(be, seed):
    cm = compile_model(random_many_dof_model(seed))
    assert 64 < cm.nv <= MAX_DOFS and cm.npair > 0 and cm.ncon > cm.npair
    lim_dofs = {int(cm.t["jnt_dofadr"][j]) for j in cm.t["lim_jntid"]}
    act_dofs = {int(x) for x in cm.t["act_dofid"]}
    assert {6, cm.nv - 1} <= lim_dofs and {6, cm.nv - 1} <= act_dofs
    N = 6
    states = (*random_states(cm, N, np.random.default_rng(seed)), np.zeros((N, cm.nv)))
    ref, _, good = check_against_oracle(be, cm, states, seed, dict(qM=2e-5, qfrc_bias=2e-4, qfrc_passive=1e-5, qfrc_actuator=1e-5, qacc_smooth=5e-4, cinert=2e-5, cvel=1e-4, xpos=1e-5),
                                        dict(efc_D=1e-3, efc_aref=1e-3, efc_J=5e-4), min_good=N // 2, strict_cost=None)
    assert (ref.efc_D[good] > 0).sum() > 0, seed  # (some rows are active)


# ---------------------------------------------------------------------------------------------------------------------------------------
# placement is not arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------------


def _fits(be, cm):
    try:
        h, dims, _keep = be.model(cm)
    except Exception:  # noqa: BLE001 - mppo_model_open refuses a placement that needs more than 160 KB of LDS
        return False
    be.lib.model_close(h)
    return True


def test_placements_and_waves_are_bit_equal(be, monkeypatch):
    """The fixture's forward probe and a stretch of env steps: every MPPO_ENV_SPILL placement that fits LDS and one or two waves per workgroup
    (MPPO_ENV_WAVES) give the same bits as the default."""
    cm = load_model(HANDS)
    for k in ("MPPO_ENV_SPILL", "MPPO_ENV_WAVES", "MPPO_ENV_GENERIC"):
        monkeypatch.delenv(k, raising=False)
    _, base = probe_and_steps(be, cm, N=5, steps=4)
    tried = []
    for var, vals in (("MPPO_ENV_SPILL", ("0", "1", "3")), ("MPPO_ENV_WAVES", ("1", "2"))):
        for v in vals:
            monkeypatch.setenv(var, v)
            if _fits(be, cm):
                assert_bit_equal(base, probe_and_steps(be, cm, N=5, steps=4)[1])
                tried.append(f"{var}={v}")
            monkeypatch.delenv(var)
    assert "MPPO_ENV_SPILL=3" in tried and "MPPO_ENV_WAVES=1" in tried, tried


@pytest.mark.gpu
def test_kernel_compiled_at_start_up_equals_the_runtime_sized_kernel(tmp_path, monkeypatch):
    """minppo_amd/jit.py compiles the environment kernel for the 77-dof fixture (the dof sets' second word a compile-time constant, eight factor
    rows per lane); its layout holds four environments per wave in 151 KB of LDS, so the library attaches it - and env steps with it equal the
    run-time-sized kernel's bit for bit."""
    monkeypatch.delenv("MPPO_ENV_SPILL", raising=False)
    startup_kernel_equals_runtime_sized(load_model(HANDS), tmp_path, monkeypatch, N=256, steps=8)


# ---------------------------------------------------------------------------------------------------------------------------------------
# environment and engine
# ---------------------------------------------------------------------------------------------------------------------------------------


def test_env_steps_follow_the_env_oracle(be):
    """A few env_steps of the fixture, the kernel re-seeded from the oracle state before each (oracle/env_oracle.py): reward and done flags."""
    cm = load_model(HANDS)
    h, dims, _keep = be.model(cm)
    N, OP, R = 5, dims.obs_pad, dims.rec_dim
    rcfg = RewardCfg(height_min_z=0.8)
    env = EnvOracle(cm.t, rcfg)
    state, reset_rec, obs = be.zeros((N, R)), be.zeros((R,)), be.zeros((N, OP))
    rew, done = be.zeros((N,)), be.zeros((N,), np.uint8)
    be.lib.env_reset(h, N, be.ptr(state), be.ptr(reset_rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), None, be.stream)
    es = env.reset(N)
    np.testing.assert_allclose(be.host(obs)[:, :dims.obs_dim], es["obs"], atol=1e-4)
    rc = nat.RewardCfg(rcfg.height_min_z, rcfg.height_max_z, 2.0, 0.2, 0.5, 0.1, 4.0, 1.0, 1.25)
    rng = np.random.default_rng(4)
    n_done = 0
    for t in range(5):
        a = (0.5 * rng.standard_normal((N, cm.nu))).astype(f32)
        if t == 2:
            es["pipeline_state"]["qvel"][1, 2] = -40.0  # slammed down: ends by height
        be.put(state, pack(env, es["pipeline_state"], dims, cm.nv))
        da = be.arr(a)
        be.lib.env_step(h, N, 1, C.byref(rc), be.ptr(state), be.ptr(reset_rec), be.ptr(da), cm.nu, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), None, be.stream)
        es = env.step(es, a.astype(f64))
        got_done = be.host(done).astype(bool)
        assert (got_done == es["done"]).all(), (t, got_done, es["done"])
        n_done += int(got_done.sum())
        np.testing.assert_allclose(be.host(rew), es["reward"], atol=1e-2)
    assert n_done >= 1
    be.lib.model_close(h)


def test_engine_trains_on_the_fixture(be):
    """make_train's engine on the fixture (environment.model=...): two PPO updates (a small N on the emulator), finite losses, changed parameters.
    Its observation (952 wide) takes the float layer-wise path of the update."""
    from minppo_amd.config import load_config_from_cli

    n = ["training.num_envs=512", "training.num_minibatches=4", "training.update_epochs=2"] if be.name == "hip" else \
        ["training.num_envs=8", "training.num_minibatches=2", "training.update_epochs=1", "training.num_steps=4", "rl.num_env_steps=4"]
    cfg = load_config_from_cli(["stompy_pro", f"environment.model={HANDS}", *n, "training.total_timesteps=100000000"])
    tr = be.trainer(cfg, use_graph=False)
    assert tr.O == load_model(HANDS).obs_size() and tr.A == 61
    tr.reset()
    p0 = tr.params_flat().copy()
    for _ in range(2):
        tr.rollout()
        tr.learn()
    p1 = tr.params_flat()
    assert np.isfinite(p1).all() and np.isfinite(tr.losses()).all() and not np.array_equal(p0, p1)
    tr.close()
