"""Ball joints (MuJoCo's fourth joint type) through the MJCF parser / writer, the model compiler, the blob validator and the environment kernel:
known answers that pin the float64 oracle (oracle/physics_oracle.py) against closed forms and against models today's oracle steps along another
code path, the kernel against that reference on the emulator and the MI355X, bit-equality across kernel instantiations and Jacobian
placements, mutated blobs, and reproducible training on the ball-joint humanoid."""

import ctypes as C
import logging
from pathlib import Path

import numpy as np
import pytest

from minppo_amd import _native as nat
from minppo_amd import mjcf
from minppo_amd.model import BUILTIN_MODELS, JNT_BALL, JNT_HINGE, ActuatorSpec, JointSpec, compile_model, load_model
from oracle.physics_oracle import Physics, PhysState, quat_rotvec
from physics_harness import (SMOOTH_TOL, assert_bit_equal, assert_oracle_reproduces_the_recording, check_against_oracle, oracle_pair, probe, probe_and_steps, rot_quat,
                             start_states, startup_kernel_equals_runtime_sized, step_once, trains_reproducibly, walking_states)

f32, f64 = np.float32, np.float64
GOLDEN = Path(__file__).parent / "golden"
HUMANOID = str(GOLDEN / "ball_joints" / "ball_humanoid.xml")
CHAIN = str(GOLDEN / "ball_joints" / "ball_chain.xml")


# ---------------------------------------------------------------------------------------------------------------------------------------
# parser, writer, compiler
# ---------------------------------------------------------------------------------------------------------------------------------------

ONE_XML = """<mujoco model="one"><compiler angle="{angle}" autolimits="{auto}"/><option timestep="0.002" gravity="0 0 -9.81"/>
  <default><joint axis="0 1 0" damping="0.3"/><default class="sph"><joint type="ball" range="0 {rmax}" stiffness="2" armature="0.01"/></default></default>
  <worldbody><body name="a" pos="0 0 1" childclass="sph"><joint name="j" {jattr}/><inertial pos="0 0 -0.1" mass="1" diaginertia="0.01 0.02 0.03"/>
    {more}</body></worldbody>{tail}</mujoco>"""


def _one(angle="radian", auto="true", rmax="0.7", jattr="", more="", tail=""):
    return ONE_XML.format(angle=angle, auto=auto, rmax=rmax, jattr=jattr, more=more, tail=tail)


def test_defaults_classes_degrees_and_autolimits():
    spec = mjcf.parse_mjcf(_one())
    j = spec.bodies[0].joints[0]
    # the class (through childclass) makes it a ball joint; the axis of the enclosing default is ignored; damping is inherited
    assert j.type == JNT_BALL and j.range == (0.0, 0.7) and j.stiffness == 2.0 and j.damping == 0.3 and j.armature == 0.01 and tuple(j.axis) == (0.0, 0.0, 1.0)
    deg = mjcf.parse_mjcf(_one(angle="degree", rmax="45")).bodies[0].joints[0]
    assert deg.range[0] == 0.0 and abs(deg.range[1] - np.pi / 4) < 1e-15
    assert mjcf.parse_mjcf(_one(auto="false")).bodies[0].joints[0].range is None          # a range without limited="true"
    assert mjcf.parse_mjcf(_one(auto="false", jattr='limited="true"')).bodies[0].joints[0].range == (0.0, 0.7)
    assert mjcf.parse_mjcf(_one(jattr='limited="false"')).bodies[0].joints[0].range is None
    cm = compile_model(spec)
    assert (cm.nq, cm.nv, cm.nlimit, int(cm.t["nball"])) == (4, 3, 1, 1)
    assert list(cm.t["lim_jntid"]) == [0] and list(cm.t["dof_jntid"]) == [0, 0, 0] and list(cm.t["dof_damping"]) == [0.3] * 3


def test_frictionloss_on_a_ball_joint_is_dropped_with_the_warning(caplog):
    with caplog.at_level(logging.WARNING, logger="minppo_amd.mjcf"):
        spec = mjcf.parse_mjcf(_one(jattr='frictionloss="0.2"'))
    assert spec.bodies[0].joints[0].type == JNT_BALL and any("frictionloss" in r.getMessage() for r in caplog.records)


@pytest.mark.parametrize("path", [HUMANOID, CHAIN])
def test_fixtures_round_trip_through_the_mjcf_writer(path):
    spec = mjcf.load_mjcf(path)
    text = mjcf.to_mjcf(spec)
    assert 'type="ball"' in text
    again = mjcf.parse_mjcf(text, name=spec.name)
    assert compile_model(again).to_blob() == compile_model(spec).to_blob()


def test_chain_tables_spelled_out():
    cm = load_model(CHAIN)
    t = cm.t
    assert (cm.nq, cm.nv, cm.nu, cm.njnt, cm.nlimit, int(t["nball"])) == (9, 7, 2, 3, 2, 2)
    assert list(t["jnt_type"]) == [JNT_BALL, JNT_BALL, JNT_HINGE] and list(t["jnt_qposadr"]) == [0, 4, 8] and list(t["jnt_dofadr"]) == [0, 3, 6]
    np.testing.assert_array_equal(t["qpos0"], [1, 0, 0, 0, 1, 0, 0, 0, 0])
    np.testing.assert_array_equal(t["qpos_spring"], [1, 0, 0, 0, 1, 0, 0, 0, 0])
    assert list(t["dof_qposadr"]) == [-1] * 6 + [8]
    assert list(t["dof_jntid"]) == [0, 0, 0, 1, 1, 1, 2] and list(t["dof_bodyid"]) == [1, 1, 1, 2, 2, 2, 3] and list(t["dof_parentid"]) == [-1, 0, 1, 2, 3, 4, 5]
    # all three cdof_dot of a ball joint use the velocity accumulated BEFORE the joint: nothing, dofs 0-2, dofs 0-5
    assert [int(np.uint32(x)) for x in np.asarray(t["dof_velmask"]).reshape(-1, 2)[:, 0]] == [0, 0, 0, 7, 7, 7, 63]
    # dof_invweight0: the mean of diag(M^-1) over each ball joint's three dofs (MuJoCo averages them, as for a free joint's triples)
    dinv = np.diag(np.linalg.inv(t["M0"]))
    np.testing.assert_allclose(t["dof_invweight0"], [dinv[:3].mean()] * 3 + [dinv[3:6].mean()] * 3 + [dinv[6]], rtol=1e-13)
    assert not np.allclose(dinv[:3], dinv[:3].mean())
    # the motor on the ball joint: the gear vector in the actuator's bias row, gear 0, gain 1; the hinge's motor as ever
    np.testing.assert_array_equal(t["act_bias"], [[0.3, 0.5, -0.2], [0, 0, 0]])
    assert list(t["act_gear"]) == [0.0, 1.0] and list(t["act_gain"]) == [1.0, 1.0] and list(t["act_dofid"]) == [3, 6]
    np.testing.assert_array_equal(t["jnt_range"], [[0, 0.9], [0, 0], [-1.5, 1.5]])


HAND_XML = """<mujoco model="m"><compiler angle="radian"/><worldbody>
  <body name="a" pos="0 0 1"><joint name="j" type="ball" {jattr}/>{j2}<inertial pos="0 0 -0.1" mass="1" diaginertia="0.01 0.02 0.03"/>
    <body name="b" pos="0 0 -0.2"><joint name="h" axis="0 1 0"/><inertial pos="0 0 -0.1" mass="1" diaginertia="0.01 0.02 0.03"/></body></body>
  </worldbody>{tail}</mujoco>"""


@pytest.mark.parametrize("kw,msg", [
    (dict(jattr='range="-1.57 0"'), r"joint j: joint type 'ball' takes range=\"0 max\""),
    (dict(jattr='range="0.2 1"'), r"joint j: joint type 'ball'"),
    (dict(jattr='range="0 0"'), r"joint j: joint type 'ball'"),
    (dict(jattr='ref="0.1"'), r"joint j: ref / springref"),
    (dict(jattr='springref="0.1"'), r"joint j: ref / springref"),
    (dict(j2='<joint name="k" axis="1 0 0"/>'), r"ball joint 'j' must be the only joint of its body.*'k'"),
    (dict(tail='<equality><joint joint1="j" joint2="h"/></equality>'), r"joint1 'j' is a ball joint"),
    (dict(tail='<equality><joint joint1="h" joint2="j"/></equality>'), r"joint2 'j' is a ball joint"),
    (dict(tail='<actuator><position name="p" joint="j" kp="3"/></actuator>'), r"position name='p' joint='j'.*ball joint"),
    (dict(tail='<actuator><velocity name="v" joint="j"/></actuator>'), r"velocity name='v' joint='j'.*ball joint"),
    (dict(tail='<actuator><general name="g" joint="j" biastype="affine" biasprm="0 -1 0"/></actuator>'), r"general name='g' joint='j'.*ball joint"),
])
def test_refusals_name_the_element(kw, msg):
    xml = HAND_XML.format(jattr=kw.get("jattr", ""), j2=kw.get("j2", ""), tail=kw.get("tail", ""))
    with pytest.raises(ValueError, match=msg):
        compile_model(mjcf.parse_mjcf(xml))


def test_compiler_refuses_what_the_parser_cannot_see():
    spec = mjcf.parse_mjcf(HAND_XML.format(jattr="", j2="", tail=""))
    spec.actuators = [ActuatorSpec("j", gear=2.0)]
    with pytest.raises(ValueError, match="ball joint j: gear needs three components"):
        compile_model(spec)
    spec.actuators = [ActuatorSpec("j", gear=(1.0, 0.0, 0.0), kp=5.0)]
    with pytest.raises(ValueError, match="ball joint j: only a motor"):
        compile_model(spec)
    spec.actuators = []
    spec.bodies[0].joints[0].range = (-0.5, 0.5)
    with pytest.raises(ValueError, match="joint j: joint type 'ball' takes range"):
        compile_model(spec)
    spec.bodies[0].joints[0].range = None
    spec.bodies[0].joints.append(JointSpec("k", JNT_HINGE))
    with pytest.raises(ValueError, match="ball joint 'j' must be the only joint of its body"):
        compile_model(spec)


def _models_without_ball_joints():
    out = [(n, lambda f=f: compile_model(f())) for n, f in sorted(BUILTIN_MODELS.items())]
    for p in sorted(list(GOLDEN.glob("*.xml")) + [GOLDEN / "export_biped" / "robot.xml"] + list((GOLDEN / "equality").glob("*.xml"))):
        out.append((str(p.relative_to(GOLDEN)), lambda p=p: load_model(str(p))))
    return out


def test_oracle_reproduces_the_recording_without_ball_joints():
    """Ball joints change nothing for a model without one: the oracle on every built-in robot and every earlier fixture against the recording
    made before it knew the joint type."""
    models = _models_without_ball_joints()
    for name, make in models:
        assert "nball" not in make().t, name
    assert_oracle_reproduces_the_recording([n for n, _ in models])


# ---------------------------------------------------------------------------------------------------------------------------------------
# known answers on the reference (float64): closed forms, and models that today's oracle steps along another code path
# ---------------------------------------------------------------------------------------------------------------------------------------

I123 = (0.011, 0.023, 0.037)
TOP_XML = """<mujoco model="top"><option timestep="0.001" gravity="0 0 {g}"/><worldbody>
  <body name="top" pos="0 0 1">{joint}<inertial pos="{ipos}" mass="1.3" diaginertia="{I}"/></body></worldbody></mujoco>"""


def _top(joint, g="0", ipos="0 0 0", I=I123):
    return compile_model(mjcf.parse_mjcf(TOP_XML.format(joint=joint, g=g, ipos=ipos, I=" ".join(map(str, I)))))


def _state(ph, qpos, qvel, ctrl=None):
    N = qpos.shape[0]
    d = PhysState(qpos=np.asarray(qpos, f64).copy(), qvel=np.asarray(qvel, f64).copy(), ctrl=np.zeros((N, ph.nu)) if ctrl is None else np.asarray(ctrl, f64),
                  qacc_warmstart=np.zeros((N, ph.nv)), time=np.zeros(N))
    ph.forward(d)
    return d


def test_eulers_equations():
    """One body on a ball joint at its centre of mass, no gravity: I dw/dt = -(w x I w), componentwise, whatever the orientation."""
    cm = _top('<joint name="j" type="ball"/>')
    ph = Physics(cm.t)
    rng = np.random.default_rng(0)
    N = 16
    q = rot_quat(rng.standard_normal((N, 3)))
    w = 3.0 * rng.standard_normal((N, 3))
    d = _state(ph, q, w)
    I = np.asarray(I123)
    want = -np.cross(w, I * w) / I
    assert np.abs(d.qacc - want).max() <= 1e-12 * np.abs(want).max()


def test_ball_at_the_centre_of_mass_is_a_free_body_at_rest():
    """The same body on a free joint with zero linear velocity (no gravity, no plane), stepped by oracle.physics_oracle.Physics as it
    stands: orientation and angular velocity follow each other over 500 steps (the same discrete map through different code).
    Measured: 0 (the two paths round alike)."""
    ball, free = _top('<joint name="j" type="ball"/>'), _top("<freejoint/>")
    pb, pf = Physics(ball.t), Physics(free.t)
    rng = np.random.default_rng(1)
    N = 4
    q = rot_quat(rng.standard_normal((N, 3)))
    w = 4.0 * rng.standard_normal((N, 3))
    db = pb.pipeline_init(q, w)
    df = pf.pipeline_init(np.concatenate([np.zeros((N, 2)), np.ones((N, 1)), q], 1), np.concatenate([np.zeros((N, 3)), w], 1))
    worst = 0.0
    for _ in range(500):
        db, df = pb.pipeline_step(db, np.zeros((N, 0))), pf.pipeline_step(df, np.zeros((N, 0)))
        worst = max(worst, np.abs(db.qpos - df.qpos[:, 3:7]).max(), np.abs(db.qvel - df.qvel[:, 3:6]).max())
    print("ball / free body deviation over 500 steps:", worst)
    assert worst <= 1e-9
    assert np.abs(df.qvel[:, :3]).max() <= 1e-12  # (the free body stays at rest: the comparison is the rotational one)


def test_planar_ball_is_a_hinge():
    """A ball pendulum under gravity released with angular velocity about the body y axis only, against the same pendulum on a y hinge
    (today's oracle): the rotation angle of the ball's quaternion is the hinge angle over 500 steps of 1 ms.  Measured: 1.2e-14, nothing out of the plane."""
    ball = _top('<joint name="j" type="ball" pos="0 0 0.25"/>', g="-9.81")
    hinge = _top('<joint name="j" type="hinge" axis="0 1 0" pos="0 0 0.25"/>', g="-9.81")
    pb, ph = Physics(ball.t), Physics(hinge.t)
    th0, w0 = np.array([0.4, -1.1]), np.array([1.5, 0.3])
    db = pb.pipeline_init(rot_quat(np.stack([0 * th0, th0, 0 * th0], 1)), np.stack([0 * w0, w0, 0 * w0], 1))
    dh = ph.pipeline_init(th0[:, None], w0[:, None])
    worst = off = 0.0
    for _ in range(500):
        db, dh = pb.pipeline_step(db, np.zeros((2, 0))), ph.pipeline_step(dh, np.zeros((2, 0)))
        ang = 2.0 * np.arctan2(db.qpos[:, 2], db.qpos[:, 0])
        worst = max(worst, np.abs(ang - dh.qpos[:, 0]).max(), np.abs(db.qvel[:, 1] - dh.qvel[:, 0]).max())
        off = max(off, np.abs(db.qvel[:, [0, 2]]).max(), np.abs(db.qpos[:, [1, 3]]).max())
    print("ball / hinge deviation over 500 steps:", worst, "out of plane:", off)
    assert worst <= 1e-9 and off <= 1e-12
    assert np.abs(dh.qpos[:, 0] - th0).max() > 0.3  # (it did swing)


TREE_XML = """<mujoco model="tree"><option timestep="0.002"/><worldbody><geom type="plane" size="0 0 1" contype="1" conaffinity="1"/>
  <body name="a" pos="0.1 0 0.5" quat="0.8 0.3 -0.4 0.33">{joints}<inertial pos="0.02 0.01 -0.1" mass="1.1" diaginertia="0.012 0.02 0.008" quat="0.9 0.1 0.3 0.2"/>
    <body name="b" pos="0.05 0 -0.25" quat="0.95 0.1 0.2 0"><joint name="h" axis="0.3 1 0.2" pos="0.01 0 0"/><inertial pos="0 0.02 -0.1" mass="0.7" diaginertia="0.004 0.005 0.002"/>
      <geom type="sphere" size="0.4" pos="0 0 -0.1" contype="1" conaffinity="0" mass="0"/>
      <geom type="capsule" size="0.05 0.3" pos="0.1 0 -0.1" quat="0.7 0.7 0 0" contype="1" conaffinity="0" mass="0"/></body></body>
  </worldbody></mujoco>"""


def test_ball_is_three_coincident_hinges_at_qpos0():
    """A subtree with ground contacts hung from a body on a ball joint, against the same model with three hinges x, y, z at that anchor, at
    qpos0 and at rest: mass matrix, bias force, smooth acceleration, poses and contact rows.  Measured: 0 in every quantity."""
    ball = compile_model(mjcf.parse_mjcf(TREE_XML.format(joints='<joint name="s" type="ball" pos="0.02 -0.01 0.03"/>')))
    three = compile_model(mjcf.parse_mjcf(TREE_XML.format(joints="".join(f'<joint name="s{k}" type="hinge" pos="0.02 -0.01 0.03" axis="{a}"/>' for k, a in enumerate(("1 0 0", "0 1 0", "0 0 1"))))))
    assert ball.nv == three.nv == 4 and ball.ncon == three.ncon == 3
    db = _state(Physics(ball.t), np.asarray(ball.t["qpos0"])[None], np.zeros((1, 4)))
    dh = _state(Physics(three.t), np.asarray(three.t["qpos0"])[None], np.zeros((1, 4)))
    assert (db.efc_D > 0).sum() >= 4 and np.array_equal(db.efc_D > 0, dh.efc_D > 0)  # (the sphere touches the ground)
    for k in ("qM", "qfrc_bias", "qacc_smooth", "xpos", "efc_J", "efc_D", "efc_aref", "qacc"):
        dev = np.abs(db[k] - dh[k]).max() / (np.abs(dh[k]).max() + 1e-300)
        print(k, dev)
        assert dev <= 1e-10, (k, dev)


LIMIT_XML = """<mujoco model="lim"><compiler angle="radian"/><option timestep="0.002" gravity="0 0 0"/><worldbody>
  <body name="a" pos="0 0 1"><joint name="j" type="ball" range="0 {rmax}" {jattr}/><inertial pos="0.02 0 -0.1" mass="1" diaginertia="0.01 0.02 0.03"/></body>
  </worldbody>{tail}</mujoco>"""


@pytest.mark.parametrize("rmax,margin", [(0.8, 0.0), (0.8, 0.05), (2.0, 0.0)])
def test_limit_row(rmax, margin):
    """theta > theta_max: one active row, Jacobian -u on the three dofs, pos = theta_max - theta - margin; theta < theta_max - margin: inert;
    theta near pi and the quaternion's other sign (the wrap)."""
    cm = compile_model(mjcf.parse_mjcf(LIMIT_XML.format(rmax=rmax, jattr=f'margin="{margin}" solreflimit="0.03 0.9"' if margin else "", tail="")))
    assert cm.nlimit == 1 and int(cm.t["cparam"]) == (1 if margin else 0)
    ph = Physics(cm.t)
    rng = np.random.default_rng(2)
    u = rng.standard_normal((6, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    theta = np.array([rmax + 0.3, rmax + 0.01, rmax - margin - 0.01, 0.1, 3.1, rmax - 0.5 * margin if margin else rmax + 1e-3])
    for sign in (1.0, -1.0):
        w = rng.standard_normal((6, 3))
        d = _state(ph, sign * rot_quat(u * theta[:, None]), w)
        pos = rmax - theta - margin
        act = pos < 0
        assert list(act) == [True, True, False, False, True, True]
        np.testing.assert_allclose(d.efc_J[:, 0], np.where(act[:, None], -u, 0.0), atol=1e-12)
        sr, si = (cm.t["lim_solref"][0], cm.t["lim_solimp"][0]) if margin else (cm.t["limit_solref"], cm.t["limit_solimp"])
        k, b, imp = ph._kbi(sr, si, pos)
        R = cm.t["dof_invweight0"][0] * (1 - imp) / imp
        np.testing.assert_allclose(d.efc_D[:, 0], np.where(act, 1 / R, 0.0), rtol=1e-12)
        assert (d.efc_D[~act, 0] == 0).all()
        np.testing.assert_allclose(d.efc_aref[:, 0], np.where(act, -b * np.sum(-u * w, 1) - k * imp * pos, 0.0), rtol=1e-10, atol=1e-10)


def test_spring_and_motor():
    """qfrc_passive = -k theta u on the three dofs (plus damping); qfrc_actuator = gain * ctrl * gear, clamped by ctrlrange, forcerange and
    per dof by actuatorfrcrange."""
    tail = '<actuator><general name="m" joint="j" gear="2 -3 0.5" gainprm="4" ctrlrange="-1 1" ctrllimited="true" forcerange="-3 3" forcelimited="true"/></actuator>'
    cm = compile_model(mjcf.parse_mjcf(LIMIT_XML.format(rmax=3.0, jattr='stiffness="2.5" damping="0.1" actuatorfrcrange="-7 7" actuatorfrclimited="true"', tail=tail)))
    ph = Physics(cm.t)
    rng = np.random.default_rng(3)
    N = 8
    u = rng.standard_normal((N, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    theta = rng.uniform(0.05, 2.9, N)
    w = rng.standard_normal((N, 3))
    ctrl = np.array([0.2, -0.5, 0.7, 0.9, -1.0, 1.7, -2.0, 0.0])[:, None]
    d = _state(ph, rot_quat(u * theta[:, None]) * np.where(np.arange(N) % 2, -1.0, 1.0)[:, None], w, ctrl)
    np.testing.assert_allclose(d.qfrc_passive, -2.5 * theta[:, None] * u - 0.1 * w, atol=1e-12)
    force = np.clip(4.0 * np.clip(ctrl, -1, 1), -3, 3)
    want = np.clip(force * np.array([2.0, -3.0, 0.5]), -7, 7)
    np.testing.assert_allclose(d.qfrc_actuator, want, atol=1e-13)
    assert (np.abs(want) == 7).any() and (np.abs(force) == 3).any()


def test_pendulum_dropped_beyond_its_limit_comes_to_rest_inside():
    xml = """<mujoco model="drop"><compiler angle="radian"/><option timestep="0.002"/><worldbody>
      <body name="a" pos="0 0 1"><joint name="j" type="ball" range="0 0.8" stiffness="0.5" damping="0.08"/><inertial pos="0 0 -0.2" mass="1" diaginertia="0.01 0.012 0.004"/></body>
      </worldbody></mujoco>"""
    cm = compile_model(mjcf.parse_mjcf(xml))
    ph = Physics(cm.t)
    d = ph.pipeline_init(rot_quat(np.array([[1.2, 0.3, 0.2], [-0.7, 1.0, -0.4]])), np.zeros((2, 3)))
    assert (d.efc_D > 0).all()  # released beyond the limit
    worst = 0.0
    for _ in range(4000):
        d = ph.pipeline_step(d, np.zeros((2, 0)))
        worst = max(worst, np.abs(np.linalg.norm(d.qpos, axis=1) - 1).max())
    ang = np.linalg.norm(quat_rotvec(d.qpos), axis=1)
    assert worst <= 1e-12 and np.isfinite(d.qpos).all()
    assert (ang < 0.05).all() and np.abs(d.qvel).max() < 0.02, (ang, d.qvel)  # hanging straight down, at rest, inside the limit


# ---------------------------------------------------------------------------------------------------------------------------------------
# the kernel against the reference (emulator here, the MI355X under -m gpu)
# ---------------------------------------------------------------------------------------------------------------------------------------


def _ball_adr(cm):
    return [(int(cm.t["jnt_qposadr"][j]), int(cm.t["jnt_dofadr"][j])) for j in range(cm.njnt) if int(cm.t["jnt_type"][j]) == JNT_BALL]


def test_kernel_follows_the_reference_on_the_fixtures(be):
    for path in (HUMANOID, CHAIN):
        cm = load_model(path)
        for s in range(2):
            ref, got, _ = check_against_oracle(be, cm, walking_states(cm, 12, s), f"{Path(path).name}/{s}", SMOOTH_TOL, dict(efc_J=1e-5, efc_D=5e-4, efc_aref=5e-4), min_good=6,
                                               strict_cost=True)
            # the spring on the quaternion and the three-component gear, relative to each quantity's largest magnitude.  qfrc_actuator is a product of three
            # float32 numbers and a sum of at most three such terms (a few 1.2e-7 roundings): 1e-6.  qfrc_passive goes through sqrtf / atan2f / a division on
            # float32 inputs before the stiffness multiplies it - the bound of the other quantity built from single-precision transcendentals here, qM: 2e-5
            for k, tol in dict(qfrc_passive=2e-5, qfrc_actuator=1e-6).items():  # (the spring on the quaternion, the three-component gear)
                assert np.abs(got[k] - ref[k]).max() <= tol * (np.abs(ref[k]).max() + 1e-6), (path, k)


def random_ball_model(seed: int):
    """tests/test_model_fuzz.py's random robot with some of its single-hinge bodies turned into ball joints - limited, sprung, damped and
    motor-actuated at random; at least one."""
    from test_model_fuzz import random_model

    spec = random_model(seed)
    rng = np.random.default_rng(9000 + seed)
    cand = [b for b in spec.bodies if len(b.joints) == 1 and b.joints[0].type == JNT_HINGE]
    assert cand, seed
    picks = [b for b in cand if rng.random() < 0.5] or [cand[int(rng.integers(len(cand)))]]
    for b in picks:
        old = b.joints[0]
        b.joints[0] = JointSpec(old.name, JNT_BALL, pos=old.pos, range=(0.0, float(rng.uniform(0.1, 1.2))) if rng.random() < 0.6 else None, damping=old.damping,
                                armature=old.armature, stiffness=float(rng.uniform(1.0, 20.0)) if rng.random() < 0.5 else 0.0,
                                actuatorfrcrange=old.actuatorfrcrange, margin=float(rng.uniform(0.0, 0.05)) if rng.random() < 0.3 else 0.0)
        spec.actuators = [a for a in spec.actuators if a.joint != old.name]
        for _ in range(int(rng.integers(0, 3))):
            spec.actuators.append(ActuatorSpec(old.name, gear=tuple(rng.uniform(-3, 3, 3)), gain=float(rng.uniform(0.5, 5.0)) if rng.random() < 0.5 else None,
                                               ctrlrange=(-1.0, 1.0) if rng.random() < 0.7 else None, forcerange=(-2.0, 2.0) if rng.random() < 0.3 else None))
    return spec


BALL_SEEDS = list(range(8))


def test_kernel_follows_the_reference_on_random_robots(be):
    for seed in BALL_SEEDS:
        cm = compile_model(random_ball_model(seed))
        assert int(cm.t["nball"]) >= 1
        check_against_oracle(be, cm, walking_states(cm, 8, seed), f"random/{seed}", SMOOTH_TOL, dict(efc_D=1e-3, efc_aref=1e-3, efc_J=5e-4), min_good=4, strict_cost=False)


def test_ball_limit_row_of_the_kernel(be):
    """States placed past the limit (not left to the walk): the kernel's active set is the reference's, its rows within the efc_J tolerance."""
    for path in (CHAIN, HUMANOID):
        cm = load_model(path)
        rng = np.random.default_rng(5)
        N = 12
        q = start_states(cm, N, rng)
        lim = [int(j) for j in cm.t["lim_jntid"] if int(cm.t["jnt_type"][j]) == JNT_BALL]
        assert lim
        for j in lim:
            qa, rmax = int(cm.t["jnt_qposadr"][j]), float(cm.t["jnt_range"][j, 1])
            u = rng.standard_normal((N, 3))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            theta = rmax + rng.uniform(-0.3, 0.6, N)  # on both sides of the limit
            q[:, qa:qa + 4] = rot_quat(u * theta[:, None]) * np.where(rng.random(N) < 0.5, -1.0, 1.0)[:, None]
        q32 = [x.astype(f32) for x in (q, 0.3 * rng.standard_normal((N, cm.nv)), np.zeros((N, max(cm.nu, 1))), np.zeros((N, cm.nv)))]
        ref, _, good, scale = oracle_pair(cm, q32)
        assert good.sum() >= N // 2
        h, _dims, _keep = be.model(cm)
        got = probe(be, h, cm, *q32)
        be.lib.model_close(h)
        rows = [cm.neq + r for r, j in enumerate(cm.t["lim_jntid"]) if int(j) in lim]
        gD, gJ, gA = got["efc_D"].reshape(N, -1), got["efc_J"].reshape(ref.efc_J.shape), got["efc_aref"].reshape(N, -1)
        act = ref.efc_D[:, rows] > 0
        assert act.any() and (~act).any()
        assert np.array_equal((gD[:, rows] > 0)[good], act[good]), path
        assert np.abs(gJ[:, rows] - ref.efc_J[:, rows])[good].max() <= 1e-5 * scale("efc_J"), path
        assert np.abs(gD[:, rows] - ref.efc_D[:, rows])[good].max() <= 5e-4 * scale("efc_D"), path
        assert np.abs(gA[:, rows] - ref.efc_aref[:, rows])[good].max() <= 5e-4 * scale("efc_aref"), path
        assert (np.abs(np.linalg.norm(gJ[:, rows][act].reshape(-1, cm.nv), axis=1) - 1) < 1e-5).all()  # an active ball row: a unit axis


def test_env_steps_keep_ball_quaternions_normalised_and_resets_restore_identity(be):
    cm = load_model(HUMANOID)
    N = 32
    h, dims, _keep = be.model(cm)
    OP, R = dims.obs_pad, dims.rec_dim
    state, reset_rec, obs = be.zeros((N, R)), be.zeros((R,)), be.zeros((N, OP))
    rew, done = be.zeros((N,)), be.zeros((N,), np.uint8)
    be.lib.env_reset(h, N, be.ptr(state), be.ptr(reset_rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), None, be.stream)
    be.sync()
    rec0 = be.host(reset_rec).copy()
    adr = _ball_adr(cm)
    assert len(adr) == 4
    for qa, _ in adr:
        assert list(rec0[qa:qa + 4]) == [1.0, 0.0, 0.0, 0.0]
    rc = nat.RewardCfg(0.45, 2.0, 2.0, 0.2, 0.5, 0.1, 4.0, 1.0, 1.25)
    rng = np.random.default_rng(4)
    ndone = 0
    for _ in range(200):
        act = be.arr(rng.standard_normal((N, cm.nu)).astype(f32))
        be.lib.env_step(h, N, 1, C.byref(rc), be.ptr(state), be.ptr(reset_rec), be.ptr(act), cm.nu, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), None, be.stream)
        be.sync()
        s, dn = be.host(state), be.host(done).astype(bool)
        assert np.isfinite(s).all()
        for qa, _ in adr:
            assert np.abs(np.linalg.norm(s[:, qa:qa + 4], axis=1) - 1).max() <= 1e-5
            assert (s[dn, qa:qa + 4] == np.array([1.0, 0.0, 0.0, 0.0], f32)).all()  # a reset restores the identity quaternions
        assert np.array_equal(s[dn], np.tile(rec0, (int(dn.sum()), 1)))
        ndone += int(dn.sum())
    assert ndone > 0  # (random actions: it falls out of the height band now and then)
    be.lib.model_close(h)


# ---------------------------------------------------------------------------------------------------------------------------------------
# bit-equality: instantiations and Jacobian placements
# ---------------------------------------------------------------------------------------------------------------------------------------


def test_specialised_ball_humanoid_kernel_equals_the_runtime_sized_kernel(be, monkeypatch):
    cm = load_model(HUMANOID)
    monkeypatch.delenv("MPPO_ENV_GENERIC", raising=False)
    monkeypatch.delenv("MPPO_ENV_SPILL", raising=False)
    flag, spec = probe_and_steps(be, cm)
    assert flag == 1
    monkeypatch.setenv("MPPO_ENV_GENERIC", "1")
    flag, gen = probe_and_steps(be, cm)
    assert flag == 0
    assert_bit_equal(spec, gen)


@pytest.mark.parametrize("path", [HUMANOID, CHAIN])
def test_jacobian_placements_are_bit_equal(be, monkeypatch, path):
    """MPPO_ENV_SPILL=0 / 1 / 3 on the run-time-sized kernel: where the matrices live is a placement, not arithmetic - ball limit rows included."""
    cm = load_model(path)
    res = []
    for spill in ("0", "1", "3"):
        monkeypatch.setenv("MPPO_ENV_SPILL", spill)
        res.append(probe_and_steps(be, cm)[1])
    for r in res[1:]:
        assert_bit_equal(res[0], r)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the validator
# ---------------------------------------------------------------------------------------------------------------------------------------


def _dir(w, name):
    from minppo_amd.model import _BLOB_F32, _BLOB_INT, BLOB_HEADER_WORDS

    k = (_BLOB_INT + _BLOB_F32).index(name)
    return int(w[BLOB_HEADER_WORDS + 2 * k])


def test_mutated_ball_blobs_are_refused():
    from backends import get_backend

    be = get_backend("emu")
    cm = load_model(CHAIN)
    w = np.frombuffer(cm.to_blob(), np.uint8).copy().view(np.int32)
    fl = lambda x: int(np.array([x], f32).view(np.int32)[0])
    jt, qa, da, dj, rg, jn = (_dir(w, k) for k in ("jnt_type", "jnt_qposadr", "jnt_dofadr", "dof_jntid", "jnt_range", "body_jntnum"))
    muts = [(jt + 2, 1, "ball"),            # the hinge's type word becomes 1: it has no three dofs of its own
            (jt, 4, "joint type"), (jt + 1, -1, "joint type"),
            (qa + 1, 6, "ball joint address"), (da + 1, 5, "ball joint address"),
            (da + 1, 2, "dof_jntid"), (dj + 4, 2, "dof_jntid"), (dj + 2, 1, "dof_jntid"), (dj + 6, 1, "dof_jntid"),
            (rg, fl(0.1), "range"), (rg + 1, fl(0.0), "range"), (rg + 1, fl(-0.5), "range"), (rg + 1, fl(np.nan), "range"),
            (jn + 1, 2, "only joint")]
    for i, v, msg in muts:
        m = w.copy()
        assert m[i] != v
        m[i] = v
        raw = m.view(np.uint8)
        dev = be.arr(raw)
        h = C.c_void_p()
        with pytest.raises(nat.NativeError, match=msg):
            be.lib.model_open(raw.ctypes.data, raw.size, be.ptr(dev), C.byref(h))
    raw = w.view(np.uint8).copy()
    dev = be.arr(raw)
    h = C.c_void_p()
    be.lib.model_open(raw.ctypes.data, raw.size, be.ptr(dev), C.byref(h))
    be.lib.model_close(h)


@pytest.mark.parametrize("path", [CHAIN, HUMANOID])
def test_fuzzed_ball_blobs_are_refused_or_harmless(path):
    """tests/test_blob_fuzz.py's single-word mutations (header dimensions, the directory, every integer table) on the ball-joint fixtures: the
    library refuses the blob or steps it on the emulator without a fault."""
    from backends import get_backend
    from minppo_amd.model import _BLOB_INT

    be = get_backend("emu")
    words = np.frombuffer(load_model(path).to_blob(True), np.uint8).copy().view(np.int32)
    rng = np.random.default_rng(77)
    nint = len(_BLOB_INT)
    ranges = [(3, 16), (32, 37), (64, 64 + 2 * nint)] + [(int(words[64 + 2 * k]), int(words[64 + 2 * k]) + int(words[64 + 2 * k + 1])) for k in range(nint)]
    candidates = np.concatenate([np.arange(a, b) for a, b in ranges])
    values = [-1, -2, 0, 1, 2, 3, 4, 7, 63, 64, 65, 127, 128, 1000, 2 ** 31 - 1, -2 ** 31]
    accepted = refused = 0
    for _ in range(200):
        w = words.copy()
        i = int(rng.choice(candidates))
        w[i] = int(rng.choice(values)) if rng.random() < 0.7 else int(w[i]) + int(rng.choice([-1, 1]))
        if w[i] == words[i]:
            continue
        raw = w.view(np.uint8)
        dev = be.arr(raw)
        h = C.c_void_p()
        try:
            be.lib.model_open(raw.ctypes.data, raw.size, be.ptr(dev), C.byref(h))
        except nat.NativeError:
            refused += 1
            continue
        accepted += 1
        try:
            step_once(be, h)
        except nat.NativeError:
            pass
        be.lib.model_close(h)
    assert refused > 50 and accepted + refused > 150


def test_spec_dims_carry_the_number_of_ball_joints():
    from minppo_amd import build as _build

    k = _build._SPEC_KEYS.index("nball")
    assert _build.spec_dims_of(load_model(HUMANOID).t)[k] == 4 and _build.spec_dims_of(load_model("synth_stompy_pro").t)[k] == 0
    assert HUMANOID in [str(Path(p)) for p in _build.SPECIALIZED_MODELS]


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the kernel compiled at start-up, the engine
# ---------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
def test_kernel_compiled_at_start_up_equals_the_runtime_sized_kernel(tmp_path, monkeypatch):
    from minppo_amd import build as _build

    startup_kernel_equals_runtime_sized(load_model(HUMANOID), tmp_path, monkeypatch, lambda dims: dims[_build._SPEC_KEYS.index("nball")] == 4)


@pytest.mark.gpu
def test_engine_trains_on_the_ball_humanoid_reproducibly():
    """make_train on the ball-joint humanoid (environment.model=...): two runs with one seed give bit-identical parameters, no NaN, finite episode metrics."""
    trains_reproducibly(HUMANOID)
