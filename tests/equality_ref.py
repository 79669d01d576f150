"""Float64 reference of equality constraints (blob version 9): the physics of tests/contact_params_ref.py with MJX's equality rows in front
of the joint limits and contacts - connect (three rows: p1 - p2 in the world frame, jacp(p1, body1) - jacp(p2, body2)) and joint (one row:
q1 - ref1 - poly(q2 - ref2), +1 at dof1 and -dpoly/dq2 at dof2) - always active in the solver's force, cost, gradient and line search.
The impedance of an element's rows is that of the norm of its residual (MuJoCo's rule for an equality of dimension > 1).

Subclasses ContactParamPhysics and is it, bit for bit, on every model without equality constraints (tests/test_equality.py holds it so).
PARITY UNPINNED: the rules are MuJoCo's / MJX's as their documentation states them; no MuJoCo is available to compare with.
"""

from __future__ import annotations

import numpy as np

from contact_params_ref import ContactParamPhysics
from oracle.physics_oracle import MJ_MINVAL, PhysState, qrot

EQ_CONNECT, EQ_JOINT = 0, 1


class EqualityPhysics(ContactParamPhysics):
    def __init__(self, tables, dtype=np.float64, n_frames: int = 1):
        super().__init__(tables, dtype, n_frames)
        self.neq = int(self.t.get("neq", 0))
        self.nefc += self.neq

    def equality_rows(self, d: PhysState):
        """-> J [N, neq, nv], pos [N, neq], invweight [neq], the norm of each row's element residual [N, neq], element of each row."""
        t, N = self.t, d.qpos.shape[0]
        J = np.zeros((N, self.neq, self.nv), self.dtype)
        pos = np.zeros((N, self.neq), self.dtype)
        for e, kind in enumerate(t["eq_type"]):
            r0 = int(t["eq_rowadr"][e])
            o1, o2 = (int(x) for x in t["eq_obj"][e])
            if kind == EQ_CONNECT:
                a = np.asarray(t["eq_anchor"][e], self.dtype)
                p1 = d.xpos[:, o1] + qrot(d.xquat[:, o1], a[:3])
                p2 = d.xpos[:, o2] + qrot(d.xquat[:, o2], a[3:])
                pos[:, r0:r0 + 3] = p1 - p2
                J[:, r0:r0 + 3] = self.jacp(d, p1, o1) - self.jacp(d, p2, o2)
            else:
                pc = np.asarray(t["eq_polycoef"][e], self.dtype)
                qa1, da1 = int(t["jnt_qposadr"][o1]), int(t["jnt_dofadr"][o1])
                p = d.qpos[:, qa1] - t["qpos0"][qa1] - pc[0]
                J[:, r0, da1] = 1.0
                if o2 >= 0:
                    qa2, da2 = int(t["jnt_qposadr"][o2]), int(t["jnt_dofadr"][o2])
                    x = d.qpos[:, qa2] - t["qpos0"][qa2]
                    p = p - (pc[1] * x + pc[2] * x ** 2 + pc[3] * x ** 3 + pc[4] * x ** 4)
                    J[:, r0, da2] = -(pc[1] + 2 * pc[2] * x + 3 * pc[3] * x ** 2 + 4 * pc[4] * x ** 3)
                pos[:, r0] = p
        row = np.asarray(t["eq_row"])
        nrm = np.zeros_like(pos)
        for e in range(len(t["eq_type"])):
            m = row == e
            nrm[:, m] = np.sqrt(np.sum(pos[:, m] ** 2, -1, keepdims=True))
        return J, pos, np.asarray(t["eq_invweight"], self.dtype)[row], nrm, row

    def make_constraint(self, d: PhysState) -> None:
        if self.neq == 0:
            return super().make_constraint(d)
        self.nefc -= self.neq
        try:
            super().make_constraint(d)
        finally:
            self.nefc += self.neq
        t = self.t
        J, pos, invw, nrm, row = self.equality_rows(d)
        D = np.zeros_like(pos)
        aref = np.zeros_like(pos)
        jv = np.einsum("nrv,nv->nr", J, d.qvel)
        for r in range(self.neq):
            e = row[r]
            k, b, imp = self._kbi(t["eq_solref"][e], t["eq_solimp"][e], nrm[:, r])
            R = np.maximum(invw[r] * (1 - imp) / imp, MJ_MINVAL)
            D[:, r] = 1.0 / R
            aref[:, r] = -b * jv[:, r] - k * imp * pos[:, r]
        d["efc_J"] = np.concatenate([J, d.efc_J], 1)
        d["efc_D"] = np.concatenate([D, d.efc_D], 1).astype(self.dtype)
        d["efc_aref"] = np.concatenate([aref, d.efc_aref], 1).astype(self.dtype)
        d["efc_active_row"] = np.concatenate([np.ones_like(pos, bool), d.efc_active_row], 1)
        d["eq_pos"] = pos

    # -- the solver: the first neq rows are active on both signs of J qacc - aref (MJX: active.at[:ne].set(True)) ---------------------
    def _ctx_update_constraint(self, d, c):
        if self.neq == 0:
            return super()._ctx_update_constraint(d, c)
        active = c["Jaref"] < 0
        active[:, :self.neq] = True
        c["active"] = active
        c["efc_force"] = d.efc_D * -c["Jaref"] * active
        c["qfrc_constraint"] = np.einsum("nrv,nr->nv", d.efc_J, c["efc_force"])
        c["gauss"] = 0.5 * np.sum((c["Ma"] - d.qfrc_smooth) * (c["qacc"] - d.qacc_smooth), -1)
        c["prev_cost"] = c["cost"]
        c["cost"] = 0.5 * np.sum(d.efc_D * c["Jaref"] * c["Jaref"] * active, -1) + c["gauss"]

    def _ls_point(self, alpha, jaref, jv, quad, quad_gauss):
        if self.neq == 0:
            return super()._ls_point(alpha, jaref, jv, quad, quad_gauss)
        x = jaref + alpha[:, None] * jv
        active = x < 0
        active[:, :self.neq] = True
        q = np.sum(quad * active[:, None, :], -1) + quad_gauss
        cost = alpha * alpha * q[:, 2] + alpha * q[:, 1] + q[:, 0]
        d0 = 2 * alpha * q[:, 2] + q[:, 1]
        d1 = 2 * q[:, 2] + (q[:, 2] == 0) * MJ_MINVAL
        return {"alpha": alpha, "cost": cost, "d0": d0, "d1": d1}
