"""Float64 reference of ball joints: the physics of tests/equality_ref.py with MuJoCo's fourth joint type - a unit quaternion in qpos
(four coordinates), three angular dofs expressed in the body's own frame.

  kinematics : the body's local rotation is the normalised joint quaternion, about the joint anchor (the hinge's form with the rotation
               taken from qpos instead of axis / angle)
  cdof       : the three columns of the body's rotation matrix about the anchor (the free joint's rotational rows with the anchor offset)
  com_vel    : all three cdof_dot use the velocity accumulated BEFORE the joint (mj_comVel), then the three dofs are added
  passive    : stiffness acts on the rotation vector (axis x angle, angle in (-pi, pi]) of the joint quaternion (mju_subQuat against the
               identity qpos_spring; MJX passive)
  limit      : MJX _instantiate_limit_ball - angle >= 0 of the joint quaternion about whatever axis, pos = range[1] - angle - margin, the
               row is -axis on the joint's three dofs, invweight dof_invweight0[dofadr]
  actuation  : a motor's scalar force times its gear's three components (compiled into the actuator's bias row, model.py) on the three dofs,
               then actuatorfrcrange per dof
  euler      : the free joint's quaternion integration with the joint's three velocities

Subclasses EqualityPhysics and is it, bit for bit, on every model without ball joints (tests/test_ball_joints.py holds it so).
PARITY UNPINNED: the rules are MuJoCo's / MJX's as their documentation and published source state them; no MuJoCo, MJX or JAX is available
to compare with.  What pins this file instead: closed forms (Euler's equations, the limit row, the spring) and models that today's oracle
code steps along another path (a free body, a hinge pendulum, three coincident hinges) - tests/test_ball_joints.py.
"""

from __future__ import annotations

import numpy as np

from equality_ref import EqualityPhysics
from oracle.physics_oracle import (JNT_FREE, JNT_HINGE, MJ_MINVAL, PhysState, axis_angle_quat, cross_motion, qmat, qmul, qrot, quat_integrate,
                                   safe_normalize)

JNT_BALL = 1


def quat_rotvec(q):
    """Rotation vector of (unit) quaternions [..., 4]: axis x angle with the angle wrapped into (-pi, pi] (mju_quat2Vel, dt = 1)."""
    v = q[..., 1:]
    s = np.linalg.norm(v, axis=-1)
    ang = 2.0 * np.arctan2(s, q[..., 0])
    ang = np.where(ang > np.pi, ang - 2.0 * np.pi, ang)
    return v * (ang / np.where(s > 0, s, 1.0) * (s > 0))[..., None]


class BallPhysics(EqualityPhysics):
    def __init__(self, tables, dtype=np.float64, n_frames: int = 1):
        super().__init__(tables, dtype, n_frames)
        t = self.t
        self.balls = [j for j in range(self.njnt) if t["jnt_type"][j] == JNT_BALL]
        for j in self.balls:  # (the base class marks the first dof of every non-free joint as a scalar coordinate)
            self.dof_qposadr[t["jnt_dofadr"][j]] = -1

    # -- fwd_position ---------------------------------------------------------
    def kinematics(self, d: PhysState) -> None:
        if not self.balls:
            return super().kinematics(d)
        t, nb = self.t, self.nbody
        N = d.qpos.shape[0]
        dt = self.dtype
        xpos = np.zeros((N, nb, 3), dt)
        xquat = np.zeros((N, nb, 4), dt); xquat[..., 0] = 1
        xanchor = np.zeros((N, self.njnt, 3), dt)
        xaxis = np.zeros((N, self.njnt, 3), dt)
        for b in range(1, nb):
            p = t["body_parent"][b]
            pos = xpos[:, p] + qrot(xquat[:, p], t["body_pos"][b])
            quat = qmul(xquat[:, p], np.broadcast_to(t["body_quat"][b], (N, 4)))
            for j in range(t["body_jntadr"][b], t["body_jntadr"][b] + t["body_jntnum"][b]):
                qa = t["jnt_qposadr"][j]
                jt = t["jnt_type"][j]
                if jt == JNT_FREE:
                    pos = d.qpos[:, qa:qa + 3].copy()
                    quat = safe_normalize(d.qpos[:, qa + 3:qa + 7])
                    xanchor[:, j] = pos
                    xaxis[:, j] = qrot(quat, t["jnt_axis"][j])
                    continue
                anchor = pos + qrot(quat, t["jnt_pos"][j])
                axis = qrot(quat, t["jnt_axis"][j])
                xanchor[:, j], xaxis[:, j] = anchor, axis
                if jt == JNT_BALL:
                    quat = qmul(quat, safe_normalize(d.qpos[:, qa:qa + 4]))
                    pos = anchor - qrot(quat, t["jnt_pos"][j])
                    continue
                disp = d.qpos[:, qa] - t["qpos0"][qa]
                if jt == JNT_HINGE:
                    quat = qmul(quat, axis_angle_quat(np.broadcast_to(t["jnt_axis"][j], (N, 3)), disp))
                    pos = anchor - qrot(quat, t["jnt_pos"][j])
                else:
                    pos = pos + axis * disp[:, None]
            xpos[:, b], xquat[:, b] = pos, safe_normalize(quat)
        d["xpos"], d["xquat"], d["xanchor"], d["xaxis"] = xpos, xquat, xanchor, xaxis
        d["xmat"] = qmat(xquat)
        d["xipos"] = xpos + qrot(xquat, t["body_ipos"][None])
        d["ximat"] = qmat(qmul(xquat, np.broadcast_to(t["body_iquat"][None], xquat.shape)))

    def com_pos(self, d: PhysState) -> None:
        super().com_pos(d)
        t = self.t
        for j in self.balls:
            b, da = t["jnt_bodyid"][j], t["jnt_dofadr"][j]
            off = d.subtree_com[:, t["body_rootid"][b]] - d.xanchor[:, j]
            d.cdof[:, da] = 0  # (the base class wrote a slide's column there)
            for k in range(3):
                ax = d.xmat[:, b, :, k]
                d.cdof[:, da + k, :3] = ax
                d.cdof[:, da + k, 3:] = np.cross(ax, off)

    def make_constraint(self, d: PhysState) -> None:
        super().make_constraint(d)
        if not self.balls:
            return
        t = self.t
        per_row = self._per_row()
        J, D, aref, act = d.efc_J, d.efc_D, d.efc_aref, d.efc_active_row
        for r, jid in enumerate(t["lim_jntid"]):
            if t["jnt_type"][jid] != JNT_BALL:
                continue
            row = self.neq + r
            qa, da = t["jnt_qposadr"][jid], t["jnt_dofadr"][jid]
            v = quat_rotvec(safe_normalize(d.qpos[:, qa:qa + 4]))
            angle = np.linalg.norm(v, axis=-1)
            axis = v / (angle + self.dtype.type(1e-6) * (angle == 0))[:, None]  # MJX normalize_with_norm
            margin = t["lim_margin"][r] if per_row else 0.0
            pos = t["jnt_range"][jid, 1] - angle - margin
            a = pos < 0
            pos = np.where(a, pos, 0.0).astype(self.dtype)
            J[:, row] = 0
            J[:, row, da:da + 3] = np.where(a[:, None], -axis, 0.0)
            k_, b_, imp = self._kbi(t["lim_solref"][r] if per_row else t["limit_solref"], t["lim_solimp"][r] if per_row else t["limit_solimp"], pos)
            R = np.maximum(t["dof_invweight0"][da] * (1 - imp) / imp, MJ_MINVAL)
            jv = np.einsum("nv,nv->n", J[:, row], d.qvel)
            D[:, row] = np.where(a, 1.0 / R, 0.0)
            aref[:, row] = np.where(a, -b_ * jv - k_ * imp * pos, 0.0)
            act[:, row] = a

    # -- fwd_velocity -----------------------------------------------------------
    def com_vel(self, d: PhysState) -> None:
        if not self.balls:
            return super().com_vel(d)
        t, nb, nv = self.t, self.nbody, self.nv
        N = d.qpos.shape[0]
        cvel = np.zeros((N, nb, 6), self.dtype)
        cdof_dot = np.zeros((N, nv, 6), self.dtype)
        for b in range(1, nb):
            v = cvel[:, t["body_parent"][b]].copy()
            for j in range(t["body_jntadr"][b], t["body_jntadr"][b] + t["body_jntnum"][b]):
                da = t["jnt_dofadr"][j]
                if t["jnt_type"][j] == JNT_FREE:
                    for k in range(3):
                        v = v + d.cdof[:, da + k] * d.qvel[:, da + k, None]
                    for k in range(3, 6):
                        cdof_dot[:, da + k] = cross_motion(v, d.cdof[:, da + k])
                    for k in range(3, 6):
                        v = v + d.cdof[:, da + k] * d.qvel[:, da + k, None]
                elif t["jnt_type"][j] == JNT_BALL:
                    for k in range(3):
                        cdof_dot[:, da + k] = cross_motion(v, d.cdof[:, da + k])
                    for k in range(3):
                        v = v + d.cdof[:, da + k] * d.qvel[:, da + k, None]
                else:
                    cdof_dot[:, da] = cross_motion(v, d.cdof[:, da])
                    v = v + d.cdof[:, da] * d.qvel[:, da, None]
            cvel[:, b] = v
        d["cvel"], d["cdof_dot"] = cvel, cdof_dot

    def passive(self, d: PhysState) -> None:
        super().passive(d)  # (damping; the springs of scalar joints - a ball joint's dofs have no qpos address)
        t = self.t
        for j in self.balls:
            stiff = t["jnt_stiffness"][j]
            if stiff != 0:
                qa, da = t["jnt_qposadr"][j], t["jnt_dofadr"][j]
                d.qfrc_passive[:, da:da + 3] -= stiff * quat_rotvec(safe_normalize(d.qpos[:, qa:qa + 4]))

    # -- actuation ----------------------------------------------------------------
    def fwd_actuation(self, d: PhysState) -> None:
        t = self.t
        on_ball = np.asarray([t["jnt_type"][t["dof_jntid"][dof]] == JNT_BALL for dof in np.asarray(t["act_dofid"]).reshape(-1)], bool) if self.nu else np.zeros(0, bool)
        if not on_ball.any():
            return super().fwd_actuation(d)
        N = d.qpos.shape[0]
        qfrc = np.zeros((N, self.nv), self.dtype)
        ctrl = d.ctrl
        lim = t["act_ctrllimited"].astype(bool)
        ctrl = np.where(lim[None], np.clip(ctrl, t["act_ctrlrange"][:, 0], t["act_ctrlrange"][:, 1]), ctrl)
        length = t["act_gear"][None] * d.qpos[:, t["act_qposadr"]]
        velocity = t["act_gear"][None] * d.qvel[:, t["act_dofid"]]
        affine = t["act_gain"][None] * ctrl + t["act_bias"][None, :, 0] + t["act_bias"][None, :, 1] * length + t["act_bias"][None, :, 2] * velocity
        force = np.where(on_ball[None], t["act_gain"][None] * ctrl, affine)  # (on a ball joint: no length, no bias - the bias row is the gear vector)
        flim = t["act_forcelimited"].astype(bool)
        force = np.where(flim[None], np.clip(force, t["act_forcerange"][:, 0], t["act_forcerange"][:, 1]), force)
        for u in range(self.nu):
            da = t["act_dofid"][u]
            if on_ball[u]:
                qfrc[:, da:da + 3] += force[:, u, None] * t["act_bias"][u][None]
            else:
                qfrc[:, da] += force[:, u] * t["act_gear"][u]
        d["actuator_force"] = force
        rng_ = np.asarray(t["dof_actfrcrange"], self.dtype)
        qfrc = np.where(qfrc < rng_[None, :, 0], rng_[None, :, 0], np.where(qfrc > rng_[None, :, 1], rng_[None, :, 1], qfrc))
        d["qfrc_actuator"] = qfrc.astype(self.dtype)

    # -- integrator --------------------------------------------------------------
    def euler(self, d: PhysState) -> None:
        if not self.balls:
            return super().euler(d)
        t = self.t
        before = d.qpos.copy()
        super().euler(d)  # (integrates a ball joint's first coordinate as a scalar: rewritten below)
        h = self.dtype.type(self.timestep)
        for j in self.balls:
            qa, da = t["jnt_qposadr"][j], t["jnt_dofadr"][j]
            d.qpos[:, qa:qa + 4] = quat_integrate(before[:, qa:qa + 4], d.qvel[:, da:da + 3], h)
        d["qpos"] = d.qpos.astype(self.dtype)
