"""Float64 reference of per-row contact parameters (blob version 8): the oracle's physics with each constraint row's own solref / solimp,
activation below the contact slot's includemargin (pos = dist - includemargin) or the joint limit's margin (pos = dist - margin), the
single normal row of a frictionless (condim 1) contact, and plane_convex keeping hull vertices within the slot's includemargin.

Subclasses oracle.physics_oracle.Physics and changes nothing for a model whose rows all take the model-wide values (compiled table
`cparam` = 0): there it is Physics bit for bit (tests/test_contact_params.py holds it so).  PARITY UNPINNED: the rules are MuJoCo's / MJX's
as their documentation states them; no MuJoCo is available to compare with.
"""

from __future__ import annotations

import numpy as np

from oracle.physics_oracle import MJ_MINVAL, Physics, PhysState, make_frame, manifold_points, qmat, qrot


class ContactParamPhysics(Physics):
    def _per_row(self) -> bool:
        return int(self.t.get("cparam", 0)) != 0

    def collision(self, d: PhysState) -> None:
        super().collision(d)
        t = self.t
        ncvx = int(t["ncvx"]) if "ncvx" in t else 0
        if not self._per_row() or ncvx == 0 or not np.any(np.asarray(t["cvx_margin"]) != 0):
            return
        # plane_convex again for the hulls with a margin: candidates are the vertices deeper than max(-includemargin, deepest - 1 mm)
        dt = self.dtype
        N = d.qpos.shape[0]
        dist, cpos, frame = d.con_dist, d.con_pos, d.con_frame
        n = np.array([0.0, 0.0, 1.0], dt)
        slots = {int(k): c for c, k in enumerate(t["con_cvx"]) if k >= 0}
        for k in range(ncvx):
            mg = float(t["cvx_margin"][k])
            if mg == 0.0:
                continue
            b = t["cvx_body"][k]
            vert = np.asarray(t["cvx_vert"][t["cvx_vadr"][k]:t["cvx_vadr"][k + 1]], dt)
            R = qmat(d.xquat[:, b])
            nl = R[:, 2, :]
            support = (t["plane_z"] - d.xpos[:, b, 2])[:, None] - nl @ vert.T
            idx = manifold_points(vert, support > np.maximum(-mg, support.max(1) - 1e-3)[:, None], nl)
            for j in range(4):
                c = slots[4 * k + j]
                ok = ~np.any(idx[:, :j] == idx[:, j:j + 1], axis=1)
                centre = d.xpos[:, b] + qrot(d.xquat[:, b], vert[idx[:, j]])
                dist[:, c] = np.where(ok, centre[:, 2] - t["plane_z"], 1.0)
                cpos[:, c] = centre - n * (0.5 * dist[:, c])[:, None]
                frame[:, c] = make_frame(np.broadcast_to(n, (N, 3)))

    def make_constraint(self, d: PhysState) -> None:
        if not self._per_row():
            return super().make_constraint(d)
        t, nv = self.t, self.nv
        N = d.qpos.shape[0]
        dt = self.dtype
        J = np.zeros((N, self.nefc, nv), dt)
        pos = np.zeros((N, self.nefc), dt)
        invw = np.zeros((N, self.nefc), dt)
        act = np.zeros((N, self.nefc), bool)
        kk = np.zeros((N, self.nefc), dt)
        bb = np.zeros((N, self.nefc), dt)
        imp = np.ones((N, self.nefc), dt)
        row = 0
        for r, jid in enumerate(t["lim_jntid"]):
            qa, da = t["jnt_qposadr"][jid], t["jnt_dofadr"][jid]
            dmin = d.qpos[:, qa] - t["jnt_range"][jid, 0]
            dmax = t["jnt_range"][jid, 1] - d.qpos[:, qa]
            p = np.minimum(dmin, dmax) - t["lim_margin"][r]
            a = p < 0
            J[:, row, da] = np.where(a, np.where(dmin < dmax, 1.0, -1.0), 0.0)
            pos[:, row] = np.where(a, p, 0.0)
            invw[:, row] = np.where(a, t["dof_invweight0"][da], 0.0)
            act[:, row] = a
            k_, b_, i_ = self._kbi(t["lim_solref"][r], t["lim_solimp"][r], pos[:, row:row + 1])
            kk[:, row], bb[:, row], imp[:, row] = k_, b_, i_[:, 0]
            row += 1
        for c in range(self.ncon):
            b = t["con_bodyid"][c]
            mg = t["con_margin"][c]
            frictionless = int(t["con_condim"][c]) == 1
            a = d.con_dist[:, c] < mg
            jp = self.jacp(d, d.con_pos[:, c], b)
            tw = t["body_invweight0"][b, 0]
            if c >= self.ncon - self.npair:
                b1 = t["pair_body"][c - (self.ncon - self.npair)][0]
                jp = jp - self.jacp(d, d.con_pos[:, c], b1)
                tw = tw + t["body_invweight0"][b1, 0]
            jc = np.einsum("nij,njv->niv", d.con_frame[:, c], jp)
            fri = t["con_friction"][c]
            iw = tw if frictionless else (tw + fri[0] * fri[0] * tw) * 2 * fri[0] * fri[0] / t["impratio"]
            r = row
            for k in (1, 2):
                for s in (1.0, -1.0):
                    on = a & (not frictionless or r == row)  # condim 1: the normal row; three inert rows keep the slot's layout
                    Jr = jc[:, 0] if frictionless else jc[:, 0] + jc[:, k] * (s * fri[0])
                    J[:, r] = np.where(on[:, None], Jr, 0.0)
                    pos[:, r] = np.where(on, d.con_dist[:, c] - mg, 0.0)
                    invw[:, r] = np.where(on, iw, 0.0)
                    act[:, r] = on
                    k_, b_, i_ = self._kbi(t["con_solref"][c], t["con_solimp"][c], pos[:, r:r + 1])
                    kk[:, r], bb[:, r], imp[:, r] = k_, b_, i_[:, 0]
                    r += 1
            row += 4
        R = np.maximum(invw * (1 - imp) / imp, MJ_MINVAL)
        jv = np.einsum("nrv,nv->nr", J, d.qvel)
        d["efc_J"] = J
        d["efc_D"] = np.where(act, 1.0 / R, 0.0).astype(dt)
        d["efc_aref"] = np.where(act, -bb * jv - kk * imp * pos, 0.0).astype(dt)
        d["efc_active_row"] = act
