"""Differential test over RANDOM robots: the three implementations of the physics step (NumPy float64 oracle, C++ twin, environment
kernel - emulator build here, HIP with -m gpu) on models nobody tuned them for.  Random kinematic forests (a free root, further free or
world-hinged trees, welded bodies, one or two hinge / slide joints per body with random anchors, axes, limits, damping, armature,
stiffness, ref / springref), random inertial frames, colliders of every kind (sphere, capsule, cylinder, box, mesh hull) under masks that
generate round-round and round-hull pairs, position and motor actuators with gears and force limits.  Everything BEFORE the solver is
compared tightly (mass matrix, bias / passive / actuator forces, constraint rows): those do not depend on how far six CG iterations get."""
import os

import numpy as np
import pytest

from minppo_amd.model import (GEOM_BOX, GEOM_CAPSULE, GEOM_CYLINDER, GEOM_MESH, GEOM_SPHERE, JNT_FREE, JNT_HINGE, JNT_SLIDE, ActuatorSpec, BodySpec, GeomSpec, JointSpec,
                              ModelSpec, compile_model)
from oracle.physics_oracle import Physics, PhysState
from physics_harness import check_against_oracle, oracle_pair, probe, random_states

f32, f64 = np.float32, np.float64


def _unit(rng, n=3):
    x = rng.normal(size=n)
    return x / np.linalg.norm(x)


def random_model(seed: int, hull_pairs: bool = False) -> ModelSpec:
    """hull_pairs: boxes and meshes carry contype 1 as well, so that a hull meets the hulls of other bodies (MJX convex_convex, round 6) - the
    same robot otherwise (no random number is drawn for it)."""
    rng = np.random.default_rng(1000 + seed)
    hct = 1 if hull_pairs else 0
    nb = int(rng.integers(3, 13))
    bodies, acts = [], []

    def geoms(scale):
        out = []
        for _ in range(int(rng.choice([0, 1, 1, 2]))):
            kind = rng.choice(["sphere", "capsule", "cylinder", "box", "mesh"], p=[0.3, 0.3, 0.1, 0.15, 0.15])
            pos, quat = tuple(0.1 * scale * rng.normal(size=3)), tuple(_unit(rng, 4))
            fr = (float(rng.uniform(0.3, 1.2)), 0.005, 0.0001)
            if kind == "sphere":
                out.append(GeomSpec(GEOM_SPHERE, (float(rng.uniform(0.03, 0.08)),), pos=pos, friction=fr, contype=1, conaffinity=5))
            elif kind == "capsule":
                out.append(GeomSpec(GEOM_CAPSULE, (float(rng.uniform(0.02, 0.05)), float(rng.uniform(0.04, 0.12))), pos=pos, quat=quat, friction=fr, contype=1, conaffinity=5))
            elif kind == "cylinder":
                out.append(GeomSpec(GEOM_CYLINDER, (float(rng.uniform(0.03, 0.07)), float(rng.uniform(0.02, 0.08))), pos=pos, quat=quat, friction=fr, contype=0, conaffinity=4))
            elif kind == "box":
                out.append(GeomSpec(GEOM_BOX, tuple(rng.uniform(0.03, 0.1, 3)), pos=pos, quat=quat, friction=fr, contype=hct, conaffinity=1))
            else:
                v = rng.normal(size=(int(rng.integers(6, 13)), 3))
                v = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.04, 0.1, 3)
                out.append(GeomSpec(GEOM_MESH, (), pos=pos, quat=quat, friction=fr, contype=hct, conaffinity=1, vertices=tuple(map(tuple, v))))
        return out

    def inertial():
        m = float(rng.uniform(0.2, 3.0))
        a = rng.uniform(0.02, 0.12, 3)                      # a box's half sizes -> a valid inertia triple
        return m, tuple(m / 3.0 * np.array([a[1] ** 2 + a[2] ** 2, a[0] ** 2 + a[2] ** 2, a[0] ** 2 + a[1] ** 2])), tuple(0.03 * rng.normal(size=3)), tuple(_unit(rng, 4))

    def joint(name):
        jt = JNT_HINGE if rng.random() < 0.75 else JNT_SLIDE
        lim = (-float(rng.uniform(0.2, 1.2)), float(rng.uniform(0.2, 1.2))) if rng.random() < 0.6 else None
        ref = float(rng.uniform(-0.3, 0.3)) if rng.random() < 0.3 else 0.0
        return JointSpec(name, jt, pos=tuple(0.05 * rng.normal(size=3)), axis=tuple(_unit(rng)), range=lim, damping=float(rng.uniform(0.0, 1.5)) if rng.random() < 0.7 else 0.0,
                         armature=float(rng.uniform(0.0, 0.05)), stiffness=float(rng.uniform(1.0, 20.0)) if rng.random() < 0.3 else 0.0, ref=ref,
                         springref=float(rng.uniform(-0.3, 0.3)) if rng.random() < 0.3 else None,
                         actuatorfrcrange=(-float(rng.uniform(0.5, 8.0)), float(rng.uniform(0.5, 8.0))) if rng.random() < 0.3 else None)

    for b in range(nb):
        m, inert, ipos, iquat = inertial()
        name = f"b{b}"
        if b == 0:
            bodies.append(BodySpec(name, "world", mass=m, inertia=inert, ipos=ipos, iquat=iquat, joints=[JointSpec("root", JNT_FREE)], geoms=geoms(1.0)))
            continue
        if rng.random() < 0.15:   # another tree: free, or hinged / sliding on the world
            top_free = rng.random() < 0.5
            js = [JointSpec(f"{name}_free", JNT_FREE)] if top_free else [joint(f"{name}_j0")]
            bodies.append(BodySpec(name, "world", pos=(float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1)), float(rng.uniform(0.2, 0.8))), quat=tuple(_unit(rng, 4)), mass=m,
                                   inertia=inert, ipos=ipos, iquat=iquat, joints=js, geoms=geoms(1.0)))
        else:
            parent = f"b{int(rng.integers(0, b))}"
            u = rng.random()
            js = [] if u < 0.2 else [joint(f"{name}_j0")] if u < 0.85 else [joint(f"{name}_j0"), joint(f"{name}_j1")]
            bodies.append(BodySpec(name, parent, pos=tuple(0.15 * rng.normal(size=3)), quat=tuple(_unit(rng, 4)), mass=m, inertia=inert, ipos=ipos, iquat=iquat, joints=js, geoms=geoms(1.0)))
        for j in bodies[-1].joints:
            if j.type != JNT_FREE and rng.random() < 0.6:
                fr = (-float(rng.uniform(2, 30)),) if rng.random() < 0.5 else None
                u = rng.random()
                if u < 0.5:
                    acts.append(ActuatorSpec(j.name, gear=float(rng.uniform(0.5, 3.0)), kp=float(rng.uniform(2, 40)), kv=float(rng.uniform(0, 1.0)) if rng.random() < 0.3 else 0.0,
                                             ctrlrange=(-1.0, 1.0) if rng.random() < 0.7 else None, forcerange=(fr[0], -fr[0]) if fr else None))
                elif u < 0.65:   # <velocity kv> / <general biastype="affine">
                    kv = float(rng.uniform(0.1, 2.0))
                    acts.append(ActuatorSpec(j.name, gear=float(rng.uniform(0.5, 2.0)), gain=kv, bias=(0.0, 0.0, -kv), ctrlrange=(-2.0, 2.0)))
                elif u < 0.75:
                    acts.append(ActuatorSpec(j.name, gear=float(rng.uniform(0.5, 2.0)), gain=float(rng.uniform(1, 10)), bias=tuple(rng.uniform(-2, 2, 3)), forcerange=(fr[0], -fr[0]) if fr else None))
                else:
                    acts.append(ActuatorSpec(j.name, gear=float(rng.uniform(0.5, 30.0)), ctrlrange=(-1.0, 1.0), forcerange=(fr[0], -fr[0]) if fr else None))
    return ModelSpec(f"random_{seed}", bodies, acts, timestep=0.002, free_root_z=float(rng.uniform(0.15, 0.6)), plane_contype=5, plane_conaffinity=0,
                     plane_friction=(float(rng.uniform(0.5, 1.0)), 0.005, 0.0001))


SEEDS = sorted(set(range(int(os.environ.get("MPPO_FUZZ_ROBOTS", "12")))) | {17})   # (MPPO_FUZZ_ROBOTS=212: the hunt DESIGN.md section 5 reports)


@pytest.mark.parametrize("seed", SEEDS)
def test_kernel_follows_the_oracle_on_a_random_robot(be, seed):
    """Smooth dynamics on every pose; constraint rows on the poses where float32 arithmetic itself is well-conditioned (pair normals between
    nearly coincident points are not).  The solver is left out: it does not converge in six iterations on these robots (see the twin test)."""
    cm = compile_model(random_model(seed))
    # (a robot with very many contact candidates - seed 17: 114 slots, 463 constraint rows - does not fit LDS four environments to a wave: the
    # run-time-sized kernel then carries two or one per wave; until round 5 such a robot was refused)
    N = 8 if seed % 2 == 0 else 7   # (7: the last workgroup is ragged whatever the environments per wave)
    states = (*random_states(cm, N, np.random.default_rng(seed)), np.zeros((N, cm.nv)))
    check_against_oracle(be, cm, states, seed, dict(qM=2e-5, qfrc_bias=2e-4, qfrc_passive=1e-5, qfrc_actuator=1e-5, qacc_smooth=5e-4, cinert=2e-5, cvel=1e-4, xpos=1e-5),
                         dict(efc_D=1e-3, efc_aref=1e-3, efc_J=5e-4), min_good=N // 2, strict_cost=None)


HULL_SEEDS = [s_ for s_ in range(40) if compile_model(random_model(s_, True)).npair > compile_model(random_model(s_)).npair][:int(os.environ.get("MPPO_FUZZ_HULL_ROBOTS", "5"))]


@pytest.mark.parametrize("seed", HULL_SEEDS)
def test_kernel_follows_the_oracle_on_a_random_robot_with_hull_pairs(be, seed):
    """Round 6: the same random robots with their boxes and meshes allowed to meet each other (MJX convex_convex: four slots a pair, in the
    links of an articulated robot this time, not in a scene of free bodies).  Constraint rows against the oracle on the well-conditioned poses; a
    hull pair's fourth slot - an exact tie in _manifold_points between a duplicate of its first and of its second point - may be any of the
    oracle's four rows of that pair (tests/test_convex_pairs.py)."""
    cm = compile_model(random_model(seed, True))
    pg = np.asarray(cm.t["pair_geom"]).reshape(-1, 16)
    hull_first = [k for k in range(cm.npair) if pg[k, 7] != 0 and pg[k, 14] != 0 and not pg[k, 3:7].any() and pg[k, 15] == 0]
    assert hull_first, seed
    h, dims, _keep = be.model(cm)
    N = 12
    rng = np.random.default_rng(500 + seed)
    qpos, qvel, ctrl = random_states(cm, N, rng)
    q32 = [x.astype(f32) for x in (qpos, qvel, ctrl if cm.nu else np.zeros((N, 1)), np.zeros((N, cm.nv)))]
    ref, _, good, scale = oracle_pair(cm, q32)
    assert good.sum() >= N // 3, (seed, good)
    got = probe(be, h, cm, *q32)
    assert ((got["efc_D"].reshape(N, -1) > 0) == (ref.efc_D > 0))[good].all(), seed
    nlim, nplane = cm.nefc - 4 * cm.ncon, cm.ncon - cm.npair
    fourth = np.zeros(cm.nefc, bool)                       # the rows of every hull pair's fourth slot
    for k in hull_first:
        r0 = nlim + 4 * (nplane + k + 3)
        fourth[r0:r0 + 4] = True
    for k, tol in dict(efc_D=1e-3, efc_aref=1e-3, efc_J=5e-4).items():
        r, g = ref[k], got[k].reshape(ref[k].shape)
        d = np.abs(g - r).reshape(N, cm.nefc, -1).max(-1)
        assert d[good][:, ~fourth].max() <= tol * scale(k), (seed, k, d[good][:, ~fourth].max() / scale(k))
        for kk in hull_first:                              # the fourth slot: one of the oracle's four
            r0 = nlim + 4 * (nplane + kk)
            g4 = g.reshape(N, cm.nefc, -1)[good][:, r0 + 12:r0 + 16]
            r4 = r.reshape(N, cm.nefc, -1)[good][:, r0:r0 + 16].reshape(-1, 4, 4, g4.shape[-1])
            assert np.abs(g4[:, None] - r4).reshape(len(g4), 4, -1).max(-1).min(-1).max() <= tol * scale(k), (seed, k, "fourth slot of pair", kk)
    be.lib.model_close(h)


@pytest.mark.parametrize("seed", SEEDS)
def test_twin_follows_the_oracle_on_a_random_robot(seed):
    """One step of the C++ twin and of the oracle from the same states, warm start zero, on the poses without deep overlaps: the velocity change
    agrees in the bulk (the solver's float32 envelope allows a tail), positions to 2e-4."""
    from oracle.cpu_twin import RewardCfg as TwinReward, Twin

    cm = compile_model(random_model(seed))
    N = 32
    rng = np.random.default_rng(50 + seed)
    qpos, qvel, ctrl = random_states(cm, N, rng)
    qpos, qvel, ctrl = qpos.astype(f32), qvel.astype(f32), ctrl.astype(f32)
    ph = Physics(cm.t)
    d = PhysState(qpos=qpos.astype(f64), qvel=qvel.astype(f64), ctrl=ctrl.astype(f64), qacc_warmstart=np.zeros((N, cm.nv)), time=np.zeros(N))
    d = ph.pipeline_step(d, ctrl.astype(f64))
    # random joint angles fold many of these robots into themselves; where geoms overlap by more than 3 cm six CG iterations end far from the
    # optimum in ANY precision (the float32 oracle is then 2e-2 .. 1e-1 from the float64 one): those poses say nothing about the twin
    shallow = d["con_dist"].min(1) > -0.03 if cm.ncon else np.ones(N, bool)
    if shallow.sum() < 6:
        pytest.skip(f"only {int(shallow.sum())} of {N} random poses without deep overlaps")
    tw = Twin(cm, reward=TwinReward(-100.0, 100.0, 2.0, 0.2, 0.5, 0.1, 4.0, 1.0, 1.25))
    tw.reset(N)
    tw.state[:, :cm.nq] = qpos
    tw.state[:, cm.nq:cm.nq + cm.nv] = qvel
    tw.state[:, tw.obs_pad:tw.obs_pad + cm.nv] = 0
    tw.step(ctrl if cm.nu else np.zeros((N, 0), f32))
    dv = np.abs(tw.state[:, cm.nq:cm.nq + cm.nv] - d["qvel"]).max(1)
    moved = np.abs(d["qvel"] - qvel).max(1)
    rel = (dv / (moved + 0.05))[shallow]
    # The bulk agrees to float32 rounding; the tail is the unconverged solver's (measured on these robots with the kernel's probe: the
    # constraint cost the float32 solvers end at is the oracle's in the median and anywhere between 0.003 x and 200 x of it in single poses, as
    # often better as worse - a light body hitting the ground at random speed is a stiff problem for six CG iterations).
    assert np.median(rel) <= 1e-3 and np.quantile(rel, 0.6) <= 0.05, (seed, int(shallow.sum()), np.median(rel), np.quantile(rel, 0.6), rel.max())
    assert np.median(np.abs(tw.state[:, :cm.nq] - d["qpos"]).max(1)[shallow]) <= 2e-4
    tw.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_random_robot_round_trips_through_mjcf(seed):
    """Writer and parser against each other on the random robots (bodies put in document order first, as MuJoCo numbers them): every table of the
    model compiled from `parse_mjcf(to_mjcf(spec))` equals the table compiled from `spec` - joints with ref / springref / actuatorfrcrange, inertial
    frames, colliders of every kind with their masks, general / position / motor actuators, the ground plane's masks."""
    from minppo_amd import mjcf

    spec = random_model(seed)
    ordered = []

    def visit(parent):
        for b in spec.bodies:
            if b.parent == parent:
                ordered.append(b)
                visit(b.name)

    visit("world")
    spec.bodies = ordered
    a = compile_model(spec)
    b = compile_model(mjcf.parse_mjcf(mjcf.to_mjcf(spec), name=spec.name))
    assert a.t.keys() == b.t.keys()
    for k in a.t:
        np.testing.assert_allclose(np.asarray(b.t[k], dtype=np.float64), np.asarray(a.t[k], dtype=np.float64), rtol=1e-12, atol=1e-12, err_msg=f"{k} (seed {seed})")
    assert a.to_blob(True) == b.to_blob(True)
