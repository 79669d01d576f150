"""MJCF equality constraints (blob version 9): <connect> (body form) and <joint> through the parser, the compiler, the blob validator and the
environment kernel - known answers of the float64 oracle (oracle/physics_oracle.py), the kernel against it on the emulator and the MI355X,
bit-equality across kernel instantiations and Jacobian placements, and reproducible training on the four-bar biped."""

import ctypes as C
import logging
from pathlib import Path

import numpy as np
import pytest

from minppo_amd import _native as nat
from minppo_amd import mjcf
from minppo_amd.model import JNT_FREE, MAX_EQ_ROWS, EqualitySpec, compile_model, load_model
from oracle.physics_oracle import Physics
from physics_harness import (SMOOTH_TOL, assert_bit_equal, assert_oracle_reproduces_the_recording, check_against_oracle, existing_models, probe_and_steps,
                             startup_kernel_equals_runtime_sized, trains_reproducibly, walking_states)

f32, f64 = np.float32, np.float64
GOLDEN = Path(__file__).parent / "golden"
FOURBAR = str(GOLDEN / "equality" / "fourbar_biped.xml")
COUPLED = str(GOLDEN / "equality" / "coupled_joints.xml")

HANG_XML = """<mujoco model="hang"><option timestep="0.002"/>
  <worldbody><body name="bob" pos="0 0 1"><freejoint/>
    <geom type="sphere" size="0.05" mass="2" contype="0" conaffinity="0"/></body>
    <body name="other" pos="0.5 0 1"><joint name="h" axis="0 1 0"/><geom type="capsule" size="0.02 0.1" mass="1" contype="0" conaffinity="0"/>
      <body name="tip" pos="0 0 -0.1"><joint name="h2" type="slide" axis="1 0 0"/><geom type="sphere" size="0.02" mass="0.5" contype="0" conaffinity="0"/></body></body></worldbody>
  {eq}</mujoco>"""
PENDULUM_XML = """<mujoco model="pendulum"><option timestep="0.002"/>
  <worldbody><body name="bob" pos="0.3 0 1"><freejoint/><geom type="sphere" size="0.05" mass="2" contype="0" conaffinity="0"/></body></worldbody>
  <equality><connect body1="bob" anchor="-0.3 0 0"/></equality></mujoco>"""


def _hang(eq):
    return mjcf.parse_mjcf(HANG_XML.format(eq=eq))


# ---------------------------------------------------------------------------------------------------------------------------------------
# parser and compiler
# ---------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("path", [FOURBAR, COUPLED])
def test_fixtures_round_trip_through_the_mjcf_writer(path):
    spec = mjcf.load_mjcf(path)
    again = mjcf.parse_mjcf(mjcf.to_mjcf(spec), name=spec.name)
    assert again.equalities == spec.equalities
    assert compile_model(again).to_blob() == compile_model(spec).to_blob()


def test_fixture_tables():
    cm = load_model(FOURBAR)
    assert cm.neq == 6 and cm.nefc == 6 + cm.nlimit + 4 * cm.ncon
    assert list(cm.t["eq_type"]) == [0, 0] and list(cm.t["eq_rowadr"]) == [0, 3] and list(cm.t["eq_row"]) == [0, 0, 0, 1, 1, 1]
    # body2's anchor: where body1's anchor is at qpos0, in body2's frame (the rod ends 8 cm in front of the ankle)
    np.testing.assert_allclose(cm.t["eq_anchor"][0], [0, 0, -0.25, 0.08, 0, 0], atol=1e-12)
    np.testing.assert_array_equal(cm.t["eq_solref"], [[0.01, 1.0], [0.01, 1.0]])  # (the "loop" default class)
    b1, b2 = cm.t["eq_obj"][0]
    assert cm.t["eq_invweight"][0] == cm.t["body_invweight0"][b1, 0] + cm.t["body_invweight0"][b2, 0]


def test_defaults_and_inactive_elements(caplog):
    with caplog.at_level(logging.INFO, logger="minppo_amd.mjcf"):
        spec = mjcf.load_mjcf(COUPLED)
    assert [e.name for e in spec.equalities] == ["mimic_pair", "polynomial", "lock"]
    assert sum("switched_off" in r.getMessage() and "active" in r.getMessage() for r in caplog.records) == 1
    by = {e.name: e for e in spec.equalities}
    assert tuple(by["lock"].solref) == (0.005, 1.0) and tuple(by["lock"].solimp) == (0.95, 0.99, 0.001, 0.5, 2.0)
    assert tuple(by["mimic_pair"].solref) == (0.02, 1.0) and tuple(by["lock"].polycoef) == (0.01, 1.0, 0.0, 0.0, 0.0)
    cm = compile_model(spec)
    assert cm.neq == 3 and list(cm.t["eq_obj"][2]) == [cm.joint_names.index("lock"), -1]
    d1, d2 = (int(cm.t["jnt_dofadr"][cm.joint_names.index(n)]) for n in ("mimic", "drive"))
    assert cm.t["eq_invweight"][0] == cm.t["dof_invweight0"][d1] + cm.t["dof_invweight0"][d2]
    # every element inactive: no equality rows at all (and no new tables)
    off = mjcf.parse_mjcf(HANG_XML.format(eq='<equality><joint joint1="h" active="false"/></equality>'))
    assert off.equalities == [] and "neq" not in compile_model(off).t


@pytest.mark.parametrize("eq,msg", [
    ('<equality><weld body1="bob"/></equality>', "weld"),
    ('<equality><tendon tendon1="t"/></equality>', "tendon"),
    ('<equality><flex flex="f"/></equality>', "flex"),
    ('<equality><connect site1="a" site2="b"/></equality>', "site"),
    ('<equality><joint name="fine" joint1="h2" joint2="h"/><joint name="bad" joint1="h" joint2="nope"/></equality>', "'bad'.*unknown joint2 'nope'"),
    ('<equality><connect body1="ghost" anchor="0 0 0"/></equality>', "unknown body1 'ghost'"),
    ('<equality><connect body1="bob" body2="ghost" anchor="0 0 0"/></equality>', "unknown body2 'ghost'"),
    ('<equality><connect name="self" body1="bob" body2="bob" anchor="0 0 0"/></equality>', "'self'.*same body"),
    ('<equality><joint joint1="h" joint2="h"/></equality>', "same joint"),
    ('<equality><connect body1="bob" anchor="0 0 0" solref="0.02 -1"/></equality>', "solref"),
])
def test_loud_errors_name_the_element(eq, msg):
    with pytest.raises(ValueError, match=msg):
        compile_model(_hang(eq))


def test_joint_equality_on_a_free_joint_is_an_error():
    spec = _hang("")
    free = next(j.name for b in spec.bodies for j in b.joints if j.type == JNT_FREE)
    spec.equalities = [EqualitySpec("joint", free, name="onfree")]
    with pytest.raises(ValueError, match="'onfree'.*free joint"):
        compile_model(spec)


def test_more_rows_than_the_kernel_holds_is_an_error():
    n = MAX_EQ_ROWS // 3 + 1
    with pytest.raises(ValueError, match=f"{3 * n} equality constraint rows.*{MAX_EQ_ROWS}"):
        compile_model(_hang("<equality>" + '<connect body1="bob" anchor="0 0 0"/>' * n + "</equality>"))
    assert compile_model(_hang("<equality>" + '<joint joint1="h"/>' * MAX_EQ_ROWS + "</equality>")).neq == MAX_EQ_ROWS


def test_empty_equality_section_is_still_an_error():
    with pytest.raises(ValueError, match="equality"):
        _hang("<equality/>")


def test_models_without_equalities_reproduce_the_recording():
    """No new tables and the row count of before for every model without equality constraints; the oracle steps them as it did before it
    knew equality rows (the recording)."""
    models = existing_models() + [("contact_params_humanoid.xml", lambda: load_model(str(GOLDEN / "contact_params_humanoid.xml")))]
    for name, make in models:
        cm = make()
        assert not any(k == "neq" or k.startswith("eq_") for k in cm.t), name
        assert cm.neq == 0 and cm.nefc == cm.nlimit + 4 * cm.ncon, name
    assert_oracle_reproduces_the_recording([n for n, _ in models])


# ---------------------------------------------------------------------------------------------------------------------------------------
# known answers of the float64 reference
# ---------------------------------------------------------------------------------------------------------------------------------------


def _run(ph, d, steps, ctrl=None):
    for _ in range(steps):
        d = ph.pipeline_step(d, np.zeros((d.qpos.shape[0], ph.nu)) if ctrl is None else ctrl(d))
    return d


def test_body_hung_from_the_world_settles_and_swings():
    cm = compile_model(mjcf.parse_mjcf(PENDULUM_XML))
    ph = Physics(cm.t)
    assert cm.neq == 3
    # at rest under its anchor: the constraint force carries the weight (2 kg), the anchor stays put
    q = np.tile(np.asarray(cm.t["qpos0"], f64), (1, 1))
    q[0, :7] = [0.0, 0.0, 0.7, np.sqrt(0.5), 0.0, np.sqrt(0.5), 0.0]  # hanging straight down from the anchor at (0, 0, 1): body x up
    d = _run(ph, ph.pipeline_init(q, np.zeros((1, cm.nv))), 1500)
    ph.forward(d)
    np.testing.assert_allclose(d.qfrc_constraint[0, :3], [0.0, 0.0, 2 * 9.81], atol=2e-3)
    assert np.abs(d.eq_pos).max() < 2e-3  # (the soft constraint's sag under 2 kg: 1.4 mm)
    # released from the horizontal: a 30 cm pendulum swings through the bottom and the anchor residual stays small
    d = ph.pipeline_init(np.tile(np.asarray(cm.t["qpos0"], f64), (1, 1)), np.zeros((1, cm.nv)))
    worst, lowest = 0.0, 1.0
    for _ in range(250):
        d = _run(ph, d, 1)
        ph.forward(d)
        worst, lowest = max(worst, np.abs(d.eq_pos).max()), min(lowest, d.qpos[0, 2])
    assert lowest < 0.72 and worst < 0.02, (lowest, worst)


def test_mimic_pair_tracks_a_torque_on_joint2_only():
    cm = load_model(COUPLED)
    ph = Physics(cm.t)
    qa = {n: int(cm.t["jnt_qposadr"][cm.joint_names.index(n)]) for n in ("drive", "mimic", "poly_in", "poly_out", "lock")}
    d = ph.pipeline_init(np.tile(np.asarray(cm.t["qpos0"], f64), (1, 1)), np.zeros((1, cm.nv)))
    travel, worst = 0.0, 0.0
    for s in range(600):
        d = _run(ph, d, 1, ctrl=lambda d: np.array([[0.3 * np.sin(s / 60.0), 0.0, 0.0]]))
        travel, worst = max(travel, abs(d.qpos[0, qa["drive"]])), max(worst, abs(d.qpos[0, qa["mimic"]] - d.qpos[0, qa["drive"]]))
    assert travel > 0.5 and worst < 0.02 * travel, (travel, worst)
    # the locked slide joint stays at ref + 0.01 (it carries the slider's and the tip's weight)
    assert abs(d.qpos[0, qa["lock"]] - (cm.t["qpos0"][qa["lock"]] + 0.01)) < 2e-3


def test_polynomial_coupling_follows_its_polynomial():
    cm = load_model(COUPLED)
    ph = Physics(cm.t)
    qi, qo = (int(cm.t["jnt_qposadr"][cm.joint_names.index(n)]) for n in ("poly_in", "poly_out"))
    d = ph.pipeline_init(np.tile(np.asarray(cm.t["qpos0"], f64), (1, 1)), np.zeros((1, cm.nv)))
    seen, worst = [], 0.0
    for s in range(800):
        d = _run(ph, d, 1, ctrl=lambda d: np.array([[0.0, 0.6 * np.sin(s / 80.0), 0.0]]))
        x = d.qpos[0, qi]
        worst = max(worst, abs(d.qpos[0, qo] - (0.8 * x + 0.5 * x ** 2 - 0.4 * x ** 3)))
        seen.append(x)
    # (the reference: +-0.64 rad, into poly_in's limits, with the coupling off its polynomial by at most 0.027 rad)
    assert max(seen) > 0.3 and min(seen) < -0.3 and worst < 0.035, (max(seen), min(seen), worst)


def test_four_bar_loop_stays_closed_while_the_crank_is_driven():
    cm = load_model(FOURBAR)
    ph = Physics(cm.t)
    d = ph.pipeline_init(np.tile(np.asarray(cm.t["qpos0"], f64), (2, 1)), np.zeros((2, cm.nv)))
    crank = [int(cm.t["jnt_qposadr"][cm.joint_names.index(n)]) for n in ("crank_l", "crank_r")]
    ankle = [int(cm.t["jnt_qposadr"][cm.joint_names.index(n)]) for n in ("ankle_l", "ankle_r")]
    ctrl = np.zeros((2, cm.nu))
    worst, c0, a0, cmove, amove = 0.0, d.qpos[:, crank].copy(), d.qpos[:, ankle].copy(), 0.0, 0.0
    for s in range(300):
        ctrl[:, 2] = ctrl[:, 5] = np.sin(s / 25.0)
        d = _run(ph, d, 1, ctrl=lambda d: ctrl)
        ph.forward(d)
        worst = max(worst, np.abs(d.eq_pos).max())
        cmove, amove = max(cmove, np.abs(d.qpos[:, crank] - c0).max()), max(amove, np.abs(d.qpos[:, ankle] - a0).max())
    assert np.isfinite(d.qpos).all()
    assert cmove > 0.5 and amove > 0.2, (cmove, amove)  # the crank drives the ankle ... (the reference: 0.82 / 0.37 rad)
    assert worst < 0.005, worst  # ... through a loop that stays closed (the reference: 0.85 mm)                                                                     # ... through a loop that stays closed


# ---------------------------------------------------------------------------------------------------------------------------------------
# the kernel against the reference (emu and hip)
# ---------------------------------------------------------------------------------------------------------------------------------------


def random_equality_model(seed: int):
    """tests/test_model_fuzz.py's random robot with random connect and joint equalities: connects between a body and the world (anchored where
    the body is at qpos0, so that walking states start near satisfied) or between two bodies, locked joints and polynomial couplings."""
    from test_model_fuzz import random_model

    spec = random_model(seed)
    rng = np.random.default_rng(7000 + seed)
    bodies = [b.name for b in spec.bodies]
    hinge = [j.name for b in spec.bodies for j in b.joints if j.type != JNT_FREE]
    eqs = []
    for k in range(int(rng.integers(1, 4))):
        b1 = bodies[int(rng.integers(len(bodies)))]
        b2 = "" if rng.random() < 0.5 else bodies[int(rng.integers(len(bodies)))]
        if b2 == b1:
            b2 = ""
        eqs.append(EqualitySpec("connect", b1, b2, anchor=tuple(rng.uniform(-0.05, 0.05, 3)), solref=(float(rng.uniform(0.01, 0.05)), float(rng.uniform(0.7, 1.3))),
                                solimp=(0.9, 0.95, 0.001, 0.5, 2.0) if rng.random() < 0.5 else (float(rng.uniform(0.5, 0.9)), 0.97, float(rng.uniform(0.001, 0.05)), 0.5, 2.0),
                                name=f"c{k}"))
    picks = rng.permutation(hinge)
    for k in range(min(len(picks) // 2, int(rng.integers(1, 4)))):
        j1, j2 = picks[2 * k], picks[2 * k + 1]
        pc = (float(rng.uniform(-0.05, 0.05)), float(rng.uniform(-1, 1)), float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-0.3, 0.3)), 0.0)
        eqs.append(EqualitySpec("joint", j1, "" if rng.random() < 0.3 else j2, polycoef=pc, name=f"j{k}"))
    spec.equalities = eqs
    return spec


EQ_SEEDS = list(range(8))


def test_kernel_follows_the_reference_on_the_fixtures(be):
    for path in (FOURBAR, COUPLED):
        cm = load_model(path)
        for s in range(2):
            check_against_oracle(be, cm, walking_states(cm, 12, s), f"{Path(path).name}/{s}", SMOOTH_TOL, dict(efc_J=1e-5, efc_D=5e-4, efc_aref=5e-4), min_good=6, strict_cost=True)


def test_kernel_follows_the_reference_on_random_robots(be):
    for seed in EQ_SEEDS:
        cm = compile_model(random_equality_model(seed))
        assert cm.neq > 0
        check_against_oracle(be, cm, walking_states(cm, 8, seed), f"random/{seed}", SMOOTH_TOL, dict(efc_D=1e-3, efc_aref=1e-3, efc_J=5e-4), min_good=4, strict_cost=False)


# ---------------------------------------------------------------------------------------------------------------------------------------
# bit-equality: instantiations and Jacobian placements
# ---------------------------------------------------------------------------------------------------------------------------------------


def test_specialised_fourbar_kernel_equals_the_runtime_sized_kernel(be, monkeypatch):
    cm = load_model(FOURBAR)
    monkeypatch.delenv("MPPO_ENV_GENERIC", raising=False)
    monkeypatch.delenv("MPPO_ENV_SPILL", raising=False)
    flag, spec = probe_and_steps(be, cm)
    assert flag == 1
    monkeypatch.setenv("MPPO_ENV_GENERIC", "1")
    flag, gen = probe_and_steps(be, cm)
    assert flag == 0
    assert_bit_equal(spec, gen)


@pytest.mark.parametrize("path", [FOURBAR, COUPLED])
def test_jacobian_placements_are_bit_equal(be, monkeypatch, path):
    """MPPO_ENV_SPILL=0 / 1 / 3 (everything in LDS / the constraint Jacobian, equality rows included, in global memory / M too) on the
    run-time-sized kernel: the large-robot placement of the equality rows."""
    cm = load_model(path)
    res = []
    for spill in ("0", "1", "3"):
        monkeypatch.setenv("MPPO_ENV_SPILL", spill)
        res.append(probe_and_steps(be, cm)[1])
    for r in res[1:]:
        assert_bit_equal(res[0], r)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the validator: mutated version-9 blobs
# ---------------------------------------------------------------------------------------------------------------------------------------


def _eq_words(cm):
    blob = np.frombuffer(cm.to_blob(), np.uint8).copy()
    w = blob.view(np.int32)
    t = cm.t
    at = len(w) - (4 + ((cm.neq + 3) & ~3) + 32 * len(t["eq_type"]))
    return w, at


def test_mutated_equality_blobs_are_refused():
    from backends import get_backend

    be = get_backend("emu")
    cases = []
    for path in (FOURBAR, COUPLED):
        cm = load_model(path)
        w, at = _eq_words(cm)
        nel, neq = len(cm.t["eq_type"]), cm.neq
        rec = at + 4 + ((neq + 3) & ~3)
        fl = lambda i, x: (i, int(np.array([x], f32).view(np.int32)[0]))
        muts = [(38, neq + 1), (38, -1), (38, MAX_EQ_ROWS + 1), (at, 0), (at, neq + 1), (at + 4, nel), (at + 4, -1), (rec, 2), (rec + 3, 1),
                fl(rec + 4, np.nan), fl(rec + 15, -0.02), fl(rec + 17, 1.5), fl(rec + 19, 0.0), fl(rec + 22, 0.0), fl(rec + 22, np.inf)]
        if cm.t["eq_type"][0] == 0:  # connect: bodies
            muts += [(rec + 1, 0), (rec + 1, cm.nbody), (rec + 2, cm.nbody), (rec + 2, -1), (rec + 2, int(cm.t["eq_obj"][0][0]))]
        else:  # joint: joints (the free joint excluded)
            muts += [(rec + 1, -1), (rec + 1, cm.njnt), (rec + 2, cm.njnt), (rec + 2, -2), (rec + 2, int(cm.t["eq_obj"][0][0]))]
        cases += [(w, i, v) for i, v in muts]
        cases.append((w[:-1], None, None))  # a section cut short
    for w, i, v in cases:
        m = w.copy()
        if i is not None:
            assert m[i] != v
            m[i] = v
        raw = m.view(np.uint8)
        dev = be.arr(raw)
        h = C.c_void_p()
        with pytest.raises(nat.NativeError):
            be.lib.model_open(raw.ctypes.data, raw.size, be.ptr(dev), C.byref(h))
    # the unmutated blobs open
    for path in (FOURBAR, COUPLED):
        w, _ = _eq_words(load_model(path))
        raw = w.view(np.uint8).copy()
        dev = be.arr(raw)
        h = C.c_void_p()
        be.lib.model_open(raw.ctypes.data, raw.size, be.ptr(dev), C.byref(h))
        be.lib.model_close(h)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the kernel compiled at start-up, the engine
# ---------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
def test_kernel_compiled_at_start_up_equals_the_runtime_sized_kernel(tmp_path, monkeypatch):
    from minppo_amd import build as _build

    cm = load_model(FOURBAR)
    startup_kernel_equals_runtime_sized(cm, tmp_path, monkeypatch, lambda dims: dims[_build._SPEC_KEYS.index("neq")] == cm.neq == 6)


@pytest.mark.gpu
def test_engine_trains_on_the_fourbar_biped_reproducibly():
    """make_train on the four-bar biped (environment.model=...): two runs with one seed give bit-identical parameters, no NaN, finite episode metrics."""
    trains_reproducibly(FOURBAR)
