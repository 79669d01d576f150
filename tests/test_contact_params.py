"""Per-geom and per-joint contact parameters (blob version 8): MuJoCo's mixing rules in the compiler, condim 1, margin / gap, per-joint
solreflimit / solimplimit / margin - compiler known answers, the existing tables unchanged, known-answer physics and the environment kernel
against the float64 oracle (oracle/physics_oracle.py) on the emulator and the MI355X."""

import ctypes as C
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from minppo_amd import _native as nat
from minppo_amd import mjcf
from minppo_amd.model import GEOM_BOX, GEOM_MESH, JNT_FREE, compile_model, load_model, mix_contact_params
from oracle.physics_oracle import Physics, PhysState
from physics_harness import (assert_bit_equal, assert_oracle_reproduces_the_recording, check_against_oracle, existing_models, probe, random_states, startup_kernel_equals_runtime_sized,
                             trains_reproducibly)

f32, f64 = np.float32, np.float64
GOLDEN = Path(__file__).parent / "golden"
FIXTURE = str(GOLDEN / "contact_params_humanoid.xml")
NEW_TABLES = {"cparam", "con_solref", "con_solimp", "con_margin", "con_condim", "lim_solref", "lim_solimp", "lim_margin", "cvx_margin"}

BALL_XML = """<mujoco model="ball"><option timestep="0.002"/>
  <worldbody><geom name="floor" type="plane" size="0 0 1" {plane}/>
    <body name="ball" pos="0 0 {z}"><freejoint/><geom type="{type}" size="{size}" {geom}/></body></worldbody></mujoco>"""


def _ball(z=0.5, geom="", plane="", type_="sphere", size="0.1"):
    return compile_model(mjcf.parse_mjcf(BALL_XML.format(z=z, geom=geom, plane=plane, type=type_, size=size)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# compiler
# ---------------------------------------------------------------------------------------------------------------------------------------


def _p(solref=(0.02, 1.0), solimp=(0.9, 0.95, 0.001, 0.5, 2.0), solmix=1.0, condim=3, margin=0.0, gap=0.0):
    return dict(solref=solref, solimp=solimp, solmix=solmix, condim=condim, margin=margin, gap=gap)


def test_mixing_rules_known_answers():
    # equal weights: the mean; solimp mixed component by component
    r = mix_contact_params(_p(solref=(0.01, 1.0), solimp=(0.8, 0.9, 0.002, 0.5, 2.0)), _p(solref=(0.03, 0.5), solimp=(0.9, 0.95, 0.004, 0.3, 3.0)))
    np.testing.assert_allclose(r["solref"], (0.02, 0.75))
    np.testing.assert_allclose(r["solimp"], (0.85, 0.925, 0.003, 0.4, 2.5))
    # weights 3 : 1 -> mix 0.75
    r = mix_contact_params(_p(solref=(0.01, 1.0), solmix=3.0), _p(solref=(0.03, 2.0), solmix=1.0))
    np.testing.assert_allclose(r["solref"], (0.015, 1.25))
    # both weights below mjMINVAL: 0.5; one of them: that side gets weight 0
    np.testing.assert_allclose(mix_contact_params(_p(solref=(0.01, 1.0), solmix=0.0), _p(solref=(0.03, 2.0), solmix=1e-20))["solref"], (0.02, 1.5))
    np.testing.assert_allclose(mix_contact_params(_p(solref=(0.01, 1.0), solmix=0.0), _p(solref=(0.03, 2.0), solmix=2.0))["solref"], (0.03, 2.0))
    np.testing.assert_allclose(mix_contact_params(_p(solref=(0.01, 1.0), solmix=2.0), _p(solref=(0.03, 2.0), solmix=0.0))["solref"], (0.01, 1.0))
    # direct form on either side: the elementwise minimum, whatever the weights
    np.testing.assert_allclose(mix_contact_params(_p(solref=(-1000.0, -20.0), solmix=5.0), _p(solref=(0.02, 1.0)))["solref"], (-1000.0, -20.0))
    np.testing.assert_allclose(mix_contact_params(_p(solref=(-1000.0, -20.0)), _p(solref=(-500.0, -40.0)))["solref"], (-1000.0, -40.0))
    # condim: the larger; margin and gap: the larger of each, includemargin = margin - gap
    r = mix_contact_params(_p(condim=1, margin=0.01, gap=0.004), _p(condim=3, margin=0.02, gap=0.001))
    assert r["condim"] == 3 and mix_contact_params(_p(condim=1), _p(condim=1))["condim"] == 1
    assert (r["margin"], r["gap"]) == (0.02, 0.004) and r["includemargin"] == 0.02 - 0.004
    # equal sides: the stored value itself, not a recomputed mix (the same bits)
    odd = (0.1 + 0.2, 0.7)
    assert mix_contact_params(_p(solref=odd, solmix=3.0), _p(solref=odd, solmix=1.0))["solref"] == odd


def test_per_element_solref_is_mixed_per_contact_slot():
    """Two geoms that disagree on solref / solimp (refused as "per-element ... values differ" before blob version 8): each ground slot mixes
    its geom's values with the plane's own, by solmix."""
    xml = """<mujoco><worldbody><geom name="floor" type="plane" size="0 0 1" solref="0.03 1" solimp="0.8 0.9 0.002" solmix="1"/>
      <body name="a" pos="0 0 0.5"><freejoint/><geom type="sphere" size="0.1" solref="0.01 1" solmix="3"/>
        <geom type="sphere" size="0.05" pos="0.2 0 0" solref="0.02 0.5" solimp="0.95 0.99 0.001" solmix="1"/></body></worldbody></mujoco>"""
    cm = compile_model(mjcf.parse_mjcf(xml))
    t = cm.t
    assert int(t["cparam"]) == 1 and cm.ncon == 2
    np.testing.assert_allclose(t["con_solref"], [[0.75 * 0.01 + 0.25 * 0.03, 1.0], [0.025, 0.75]])
    # one solimp among the geoms that give one: it is the model's (the rule before blob version 8), the first geom takes it too
    np.testing.assert_allclose(t["contact_solimp"], (0.95, 0.99, 0.001, 0.5, 2.0))
    np.testing.assert_allclose(t["con_solimp"][0], 0.75 * np.array([0.95, 0.99, 0.001, 0.5, 2.0]) + 0.25 * np.array([0.8, 0.9, 0.002, 0.5, 2.0]))
    np.testing.assert_allclose(t["con_solimp"][1], [0.875, 0.945, 0.0015, 0.5, 2.0])
    # several solref values: none of them is the model's, which stays MuJoCo's default (the CPU twin reads the model-wide tables)
    np.testing.assert_allclose(t["contact_solref"], (0.02, 1.0))


def test_condim_margin_gap_and_the_ground_plane_as_a_geom():
    cm = _ball(geom='condim="1" margin="0.02" gap="0.005"', plane='condim="1" margin="0.01"')
    t = cm.t
    assert int(t["cparam"]) == 1
    assert list(t["con_condim"]) == [1] and t["con_margin"][0] == 0.02 - 0.005
    assert list(_ball(geom='condim="1"').t["con_condim"]) == [3]   # (the plane's default condim is 3: the larger wins)
    for bad in ('condim="4"', 'condim="6"'):
        with pytest.raises(ValueError, match="condim"):
            _ball(geom=bad)
        with pytest.raises(ValueError, match="condim"):
            _ball(plane=bad)


def test_per_joint_limit_parameters_and_defaults():
    xml = """<mujoco><default><joint solreflimit="0.04 1" solimplimit="0.8 0.9 0.003" margin="0.02"/>
        <default class="stiff"><joint solreflimit="-900 -30" margin="0"/></default></default>
      <worldbody><body name="a" pos="0 0 1"><joint name="j1" axis="0 1 0" range="-0.5 0.5"/><geom type="sphere" size="0.05" contype="0" conaffinity="0"/>
        <body name="b" pos="0 0 -0.3"><joint name="j2" class="stiff" axis="0 1 0" range="-0.4 0.4"/><geom type="sphere" size="0.05" contype="0" conaffinity="0"/>
          <body name="c" pos="0 0 -0.3"><joint name="j3" axis="0 1 0" range="-0.3 0.3" solimplimit="0.7 0.8 0.01 0.4 3" margin="0.05"/>
            <geom type="sphere" size="0.05" contype="0" conaffinity="0"/></body></body></body></worldbody></mujoco>"""
    cm = compile_model(mjcf.parse_mjcf(xml))
    t = cm.t
    assert int(t["cparam"]) == 1 and cm.nlimit == 3
    np.testing.assert_allclose(t["lim_solref"], [[0.04, 1.0], [-900.0, -30.0], [0.04, 1.0]])
    np.testing.assert_allclose(t["lim_solimp"], [[0.8, 0.9, 0.003, 0.5, 2.0], [0.8, 0.9, 0.003, 0.5, 2.0], [0.7, 0.8, 0.01, 0.4, 3.0]])
    np.testing.assert_allclose(t["lim_margin"], [0.02, 0.0, 0.05])


def test_fixture_round_trips_through_the_mjcf_writer():
    spec = mjcf.load_mjcf(FIXTURE)
    a, b = compile_model(spec), compile_model(mjcf.parse_mjcf(mjcf.to_mjcf(spec)))
    assert int(a.t["cparam"]) == 1
    for k in sorted(NEW_TABLES | {"con_friction", "con_bodyid", "pair_body", "contact_solref", "contact_solimp", "limit_solref", "limit_solimp"}):
        np.testing.assert_array_equal(a.t[k], b.t[k], err_msg=k)


def test_hull_pairs_with_a_margin_are_loud_errors():
    xml = """<mujoco><worldbody><geom name="floor" type="plane" size="0 0 1"/>
      <body name="a" pos="0 0 0.5"><freejoint/><geom type="box" size="0.1 0.1 0.1" margin="{m}"/></body>
      <body name="b" pos="0.5 0 0.5"><freejoint/><geom type="sphere" size="0.1"/></body></worldbody></mujoco>"""
    assert compile_model(mjcf.parse_mjcf(xml.format(m="0"))).npair == 1
    with pytest.raises(ValueError, match="margin"):
        compile_model(mjcf.parse_mjcf(xml.format(m="0.01")))


def _table_hashes(cm):
    out = {}
    for k, v in sorted(cm.t.items()):
        if k in NEW_TABLES:
            continue
        a = np.ascontiguousarray(v)
        out[k] = hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()
    return out


def test_existing_tables_are_byte_identical():
    """Every table the compiler produced before blob version 8, for every built-in robot and fixture: sha256 recorded from the tree before
    the change (tests/golden/table_sha256.json; the new tables are left out).  These models are all uniform (cparam 0)."""
    want = json.loads((GOLDEN / "table_sha256.json").read_text())
    models = existing_models()
    assert sorted(n for n, _ in models) == sorted(want)
    for name, make in models:
        cm = make()
        assert _table_hashes(cm) == want[name], name
        assert int(cm.t["cparam"]) == 0, name


def test_oracle_reproduces_the_recording_on_uniform_models():
    """Per-row contact parameters change nothing where every row takes the model-wide values (cparam 0): the oracle on every such model
    against the recording made before it read the per-row tables."""
    assert_oracle_reproduces_the_recording([n for n, _ in existing_models()])


# ---------------------------------------------------------------------------------------------------------------------------------------
# known-answer physics (emulator and MI355X)
# ---------------------------------------------------------------------------------------------------------------------------------------


def _forward(be, cm, qpos, qvel):
    h, dims, _keep = be.model(cm)
    N = qpos.shape[0]
    q32 = [x.astype(f32) for x in (qpos, qvel, np.zeros((N, max(cm.nu, 1))), np.zeros((N, cm.nv)))]
    got = probe(be, h, cm, *q32)
    be.lib.model_close(h)
    ref = PhysState(qpos=q32[0].astype(f64), qvel=q32[1].astype(f64), ctrl=np.zeros((N, cm.nu)), qacc_warmstart=np.zeros((N, cm.nv)), time=np.zeros(N))
    Physics(cm.t).forward(ref)
    return got, ref


def test_sphere_in_the_margin_band_is_held_up(be):
    """A sphere 1 cm above the plane (0 < dist < margin = 2 cm) gets an upward constraint force; with margin 0 it falls freely."""
    q = np.array([[0.0, 0.0, 0.11, 1.0, 0.0, 0.0, 0.0]])
    got, ref = _forward(be, _ball(geom='margin="0.02"'), q, np.zeros((1, 6)))
    assert (got["efc_D"].reshape(1, -1) > 0).all() and got["qacc"][0, 2] > 0.0
    np.testing.assert_allclose(got["qacc"][0, 2], ref.qacc[0, 2], rtol=1e-2)
    got0, _ = _forward(be, _ball(), q, np.zeros((1, 6)))
    assert not (got0["efc_D"] > 0).any()
    np.testing.assert_allclose(got0["qacc"][0], [0.0, 0.0, -9.81, 0.0, 0.0, 0.0], atol=1e-5)


def test_frictionless_capsule_keeps_its_tangential_velocity(be):
    """A condim-1 capsule lying on a condim-1 plane, 1 mm into it, sliding at 1 m/s: no tangential acceleration (one normal row per contact,
    three inert ones); the same capsule with condim 3 is braked."""
    q = np.array([[0.0, 0.0, 0.049, 0.70710678, 0.0, 0.70710678, 0.0]])
    v = np.array([[1.0, 0.3, 0.0, 0.0, 0.0, 0.0]])
    kw = dict(type_="capsule", size="0.05 0.2")
    got, ref = _forward(be, _ball(geom='condim="1"', plane='condim="1"', **kw), q, v)
    D = got["efc_D"].reshape(-1, 4)
    assert (D[:, 0] > 0).all() and (D[:, 1:] == 0).all()
    assert (got["efc_J"].reshape(-1, 4, 6)[:, 1:] == 0).all()
    assert np.abs(got["qacc"][0, :2]).max() < 1e-4 and abs(got["qacc_euler"][0, 0]) < 1e-4
    assert got["qacc"][0, 2] > 0.0
    np.testing.assert_allclose(got["efc_D"].reshape(ref.efc_D.shape), ref.efc_D, rtol=1e-3)
    got3, _ = _forward(be, _ball(**kw), q, v)
    assert got3["qacc"][0, 0] < -1.0


def test_joint_within_its_limit_margin_gets_a_limit_force(be):
    xml = """<mujoco><compiler angle="radian"/><worldbody><body name="a" pos="0 0 1"><joint name="j" axis="0 1 0" range="-0.5 0.5" margin="{m}" damping="0"/>
      <inertial pos="0 0 -0.3" mass="1" diaginertia="0.01 0.01 0.01"/></body></worldbody>
      <actuator><motor joint="j"/></actuator></mujoco>"""
    q, v = np.array([[0.45]]), np.zeros((1, 1))
    cm = compile_model(mjcf.parse_mjcf(xml.format(m="0.1")))
    got, ref = _forward(be, cm, q, v)
    assert got["efc_D"][0, 0] > 0 and got["qacc"][0, 0] < got["qacc_smooth"][0, 0] - 1.0   # pushed back from the upper end
    np.testing.assert_allclose(got["efc_aref"][0, 0], ref.efc_aref[0, 0], rtol=1e-3)
    got0, _ = _forward(be, compile_model(mjcf.parse_mjcf(xml.format(m="0"))), q, v)
    assert got0["efc_D"][0, 0] == 0
    np.testing.assert_allclose(got0["qacc"][0, 0], got0["qacc_smooth"][0, 0], rtol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the kernel against the reference: the fixture and random robots with random per-geom / per-joint parameters
# ---------------------------------------------------------------------------------------------------------------------------------------


def random_param_model(seed: int):
    """A robot of tests/test_model_fuzz.py's generator with random contact parameters on every geom, the plane and every joint.  Boxes and meshes
    meet the ground only (a margin against a hull of another body is refused)."""
    from test_model_fuzz import random_model

    spec = random_model(seed)
    rng = np.random.default_rng(500 + seed)

    def solref():
        return (-float(rng.uniform(500, 3000)), -float(rng.uniform(20, 80))) if rng.random() < 0.15 else (float(rng.uniform(0.01, 0.04)), float(rng.uniform(0.7, 1.3)))

    def solimp():
        return (float(rng.uniform(0.8, 0.95)), float(rng.uniform(0.95, 0.99)), float(rng.uniform(0.001, 0.01)), float(rng.uniform(0.3, 0.7)), float(rng.choice([2.0, 1.0, 3.0])))

    for b in spec.bodies:
        for g in b.geoms:
            if g.type in (GEOM_BOX, GEOM_MESH):
                g.conaffinity = 4
            g.solref, g.solimp = solref(), solimp()
            g.solmix = float(rng.choice([0.0, 0.5, 1.0, 3.0]))
            g.condim = int(rng.choice([1, 3]))
            g.margin = float(rng.uniform(0.0, 0.03)) if rng.random() < 0.6 else 0.0
            g.gap = float(rng.uniform(0.0, 0.5 * g.margin)) if rng.random() < 0.3 else 0.0
        for j in b.joints:
            if j.type != JNT_FREE:
                j.solreflimit, j.solimplimit = solref(), solimp()
                j.margin = float(rng.uniform(0.0, 0.08)) if rng.random() < 0.6 else 0.0
    spec.plane_solref, spec.plane_solimp, spec.plane_solmix = solref(), solimp(), float(rng.uniform(0.5, 2.0))
    spec.plane_condim = int(rng.choice([1, 3]))
    spec.plane_margin = float(rng.uniform(0.0, 0.02))
    return spec


def _fixture_states(cm, N, rng):
    """The humanoid near the ground with random joint angles: arms against legs (condim-1 self-contacts), capsules in the margin band above the
    floor, joints near and in their limit margins."""
    t = cm.t
    q = np.tile(np.asarray(t["qpos0"], f64), (N, 1))
    for j in range(cm.njnt):
        qa = int(t["jnt_qposadr"][j])
        if int(t["jnt_type"][j]) == JNT_FREE:
            continue
        lo, hi = (float(x) for x in t["jnt_range"][j])
        near = np.where(rng.random(N) < 0.5, lo, hi) + rng.uniform(-0.04, 0.04, N)
        q[:, qa] = np.where(rng.random(N) < 0.4, near, rng.uniform(lo, hi, N))
    x = np.array([1.0, 0.0, 0.0, 0.0]) + 0.3 * rng.normal(size=(N, 4))
    q[:, 3:7] = x / np.linalg.norm(x, axis=1, keepdims=True)
    ph = Physics(t)
    d = ph.make_data(N)
    d["qpos"] = q.copy()
    ph.kinematics(d); ph.com_pos(d); ph.collision(d)
    low = np.where(d["con_dist"][:, :cm.ncon - cm.npair] < 0.99, d["con_dist"][:, :cm.ncon - cm.npair], np.inf).min(1)
    q[:, 2] += rng.uniform(-0.005, 0.012, N) - low
    return q, 0.3 * rng.normal(size=(N, cm.nv)), np.zeros((N, cm.nu))


def _classes(cm, ref):
    """Which kinds of rows were active: margin-band contacts, condim-1 self-contacts, mixed-parameter floor contacts, limit-margin rows."""
    t = cm.t
    nl, nplane = cm.nlimit, cm.ncon - cm.npair
    act = ref.efc_D > 0
    cact = act[:, nl:].reshape(act.shape[0], cm.ncon, 4)[:, :, 0]
    dist = ref.con_dist
    band = cact & (dist >= 0)
    mixed = np.array([not (np.array_equal(t["con_solref"][c], t["contact_solref"]) and np.array_equal(t["con_solimp"][c], t["contact_solimp"])) for c in range(nplane)], bool)
    self1 = np.asarray(t["con_condim"])[nplane:] == 1
    lim_band = np.zeros(act.shape[0], bool)
    for r, jid in enumerate(t["lim_jntid"]):
        qa = int(t["jnt_qposadr"][jid])
        dd = np.minimum(ref.qpos[:, qa] - t["jnt_range"][jid, 0], t["jnt_range"][jid, 1] - ref.qpos[:, qa])
        lim_band |= act[:, r] & (dd >= 0)
    return dict(margin_band=int(band.sum()), condim1_self=int(cact[:, nplane:][:, self1].sum()), mixed_floor=int(cact[:, :nplane][:, mixed].sum()),
                limit_margin=int(lim_band.sum()))


def _check(be, cm, qpos, qvel, ctrl, what, tol_rows, strict_cost=True):
    """physics_harness.check_against_oracle from a zero warm start, qfrc_passive among the smooth quantities -> the classes of rows that were active."""
    ref, _, _ = check_against_oracle(be, cm, (qpos, qvel, ctrl, np.zeros((qpos.shape[0], cm.nv))), what, dict(qM=2e-5, qfrc_bias=2e-4, qfrc_passive=1e-5, qacc_smooth=5e-4, xpos=1e-5),
                                     tol_rows, qpos.shape[0] // 2, strict_cost)
    return _classes(cm, ref)


PARAM_SEEDS = list(range(8))


def test_kernel_follows_the_reference(be):
    """The fixture and eight random robots with random per-geom / per-joint parameters: the kernel's constraint rows against the float64
    reference, with every class of new row active somewhere."""
    seen = dict(margin_band=0, condim1_self=0, mixed_floor=0, limit_margin=0)
    cm = load_model(FIXTURE)
    for s in range(2):
        # (test_forward_matches_oracle's tolerances)
        for k, v in _check(be, cm, *_fixture_states(cm, 16, np.random.default_rng(s)), f"fixture/{s}", dict(efc_J=1e-5, efc_D=5e-4, efc_aref=5e-4)).items():
            seen[k] += v
    for seed in PARAM_SEEDS:
        cm = compile_model(random_param_model(seed))
        assert int(cm.t["cparam"]) == 1
        # (tests/test_model_fuzz.py's, for the same generator: pair normals between nearly coincident points)
        for k, v in _check(be, cm, *random_states(cm, 8, np.random.default_rng(seed)), f"random/{seed}", dict(efc_D=1e-3, efc_aref=1e-3, efc_J=5e-4), strict_cost=False).items():
            seen[k] += v
    assert all(v > 0 for v in seen.values()), seen


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the specialised kernels, the engine
# ---------------------------------------------------------------------------------------------------------------------------------------


def test_specialised_fixture_kernel_equals_the_runtime_sized_kernel(be, monkeypatch):
    """The fixture has an instantiation of its own in the library (csrc/spec_dims.inc, cparam = 1): bit-equal to the run-time-sized kernel."""
    cm = load_model(FIXTURE)
    N = 9
    qpos, qvel, _ = _fixture_states(cm, N, np.random.default_rng(7))
    ctrl = 0.4 * np.random.default_rng(8).standard_normal((N, cm.nu))
    q32 = [x.astype(f32) for x in (qpos, qvel, ctrl, np.zeros((N, cm.nv)))]
    res = []
    for generic in (False, True):
        if generic:
            monkeypatch.setenv("MPPO_ENV_GENERIC", "1")
        else:
            monkeypatch.delenv("MPPO_ENV_GENERIC", raising=False)
        h, dims, _keep = be.model(cm)
        flag = C.c_int32(-1)
        be.lib.model_is_specialized(h, C.byref(flag))
        assert flag.value == (0 if generic else 1)
        got = probe(be, h, cm, *q32)
        OP, R = dims.obs_pad, dims.rec_dim
        state, reset_rec, obs = be.zeros((N, R)), be.zeros((R,)), be.zeros((N, OP))
        rew, done = be.zeros((N,)), be.zeros((N,), np.uint8)
        be.lib.env_reset(h, N, be.ptr(state), be.ptr(reset_rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), None, be.stream)
        rc = nat.RewardCfg(0.95, 2.0, 2.0, 0.2, 0.5, 0.1, 4.0, 1.0, 1.25)
        r2 = np.random.default_rng(3)
        for _ in range(6):
            act = be.arr((0.8 * r2.standard_normal((N, cm.nu))).astype(f32))
            be.lib.env_step(h, N, 2, C.byref(rc), be.ptr(state), be.ptr(reset_rec), be.ptr(act), cm.nu, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), None, be.stream)
            be.sync()
        got.update(state=be.host(state).copy(), obs=be.host(obs).copy(), rew=be.host(rew).copy(), done=be.host(done).copy())
        res.append(got)
        be.lib.model_close(h)
    assert_bit_equal(res[0], res[1])


@pytest.mark.gpu
def test_kernel_compiled_at_start_up_equals_the_runtime_sized_kernel(tmp_path, monkeypatch):
    """The fixture's kernel compiled at start-up (minppo_amd/jit.py) against the run-time-sized one: the path of
    tests/test_jit.py::test_attached_kernel_equals_the_runtime_sized_kernel (the library's own instantiation is bypassed for the comparison by
    asking for the run-time-sized kernel on one handle and attaching the compiled one to the other)."""
    startup_kernel_equals_runtime_sized(load_model(FIXTURE), tmp_path, monkeypatch, lambda dims: dims[-1] == 1)


@pytest.mark.gpu
def test_engine_trains_on_the_fixture_reproducibly():
    """Five PPO updates at 1024 environments on the contact-parameter humanoid: finite parameters, and two runs with one seed agree bit for bit."""
    trains_reproducibly(FIXTURE, trainer=True)
