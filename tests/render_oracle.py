"""The renderer's reference (a plain module, imported by name): a NumPy ray caster over `minppo_amd.render.scene_arrays`, written once and run in
two precisions.

  float64  THE oracle: body poses from oracle.physics_oracle's kinematics (xpos, xquat), the visuals' and the camera's poses composed from them,
           one ray per pixel centre, the closed-form intersections of csrc/k_render.hip (a hit = the ray ENTERING a shape at t > 0; the
           discriminant from the point of closest approach), Lambert + ambient, a hard shadow ray, the 1 m checker, the sky.
  float32  the same formulas with every array in float32 (kinematics included): the restatement the depth tolerance is measured with - never the
           kernel.

`compared(...)` is the mask of pixels a test may compare: the oracle's key (geom id, checker cell parity, in shadow) is the same for the ray
through the pixel centre and the four rays tilted by DELTA = 1e-4 rad up, down, left and right."""

import numpy as np

from minppo_amd.render import CAM_TRACK, scene_arrays
from oracle.physics_oracle import Physics, PhysState, qmat

DELTA = 1e-4
LIGHT = (2.0 / 7.0, -3.0 / 7.0, 6.0 / 7.0)
AMBIENT, DIFFUSE, SHADOW_BIAS = 0.35, 0.65, 1e-3
SKY, TONE_EVEN, TONE_ODD = (0.55, 0.70, 0.90), (0.75, 0.75, 0.75), (0.45, 0.50, 0.55)
SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX, MESH = 2, 3, 4, 5, 6, 7


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def scene_of(cm, dtype):
    s = scene_arrays(cm)
    return {k: (np.asarray(v, np.float32).astype(dtype) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in s.items()}  # (the blob holds float32)


def poses(cm, s, qpos, camera, dtype):
    """-> (geom position [F, ng, 3], geom rotation [F, ng, 3, 3], camera position [F, 3], camera rotation [F, 3, 3], body xpos [F, nbody, 3])"""
    ph = Physics(cm.t, dtype)
    d = PhysState(qpos=np.asarray(np.asarray(qpos, np.float32), dtype))
    ph.kinematics(d)
    xpos, rb = d["xpos"], qmat(d["xquat"])
    gb = s["geom_body"]
    gp = xpos[:, gb] + np.einsum("fgij,gj->fgi", rb[:, gb], s["geom_pos"])
    gr = np.einsum("fgij,gjk->fgik", rb[:, gb], s["geom_mat"])
    b = int(s["cam_body"][camera])
    if int(s["cam_mode"][camera]) == CAM_TRACK:
        cp = xpos[:, b] + s["cam_pos"][camera]
        cr = np.broadcast_to(s["cam_mat"][camera], (len(xpos), 3, 3)).copy()
    else:
        cp = xpos[:, b] + np.einsum("fij,j->fi", rb[:, b], s["cam_pos"][camera])
        cr = np.einsum("fij,jk->fik", rb[:, b], s["cam_mat"][camera])
    return gp.astype(dtype), gr.astype(dtype), cp.astype(dtype), cr.astype(dtype), xpos


def camera_rays(tanhalf, W, H, dtype, tilt=(0.0, 0.0)):
    """Unit directions in the CAMERA frame [H * W, 3] through the pixel centres (MuJoCo: -z forward, +x right, +y up), optionally tilted by
    (yaw, pitch) radians about the camera's y and x axes."""
    dt = np.dtype(dtype).type
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    u = (dt(2) * (px.astype(dtype) + dt(0.5)) / dt(W) - dt(1)) * dt(tanhalf) * (dt(W) / dt(H))
    v = (dt(1) - dt(2) * (py.astype(dtype) + dt(0.5)) / dt(H)) * dt(tanhalf)
    d = np.stack([u, v, -np.ones_like(u)], -1).reshape(-1, 3)
    yaw, pitch = tilt
    if yaw or pitch:
        cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
        ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
        d = (d.astype(np.float64) @ (ry @ rx).T).astype(dtype)
    return d


class _Clip:
    def __init__(self, n, dtype):
        self.t0 = np.full(n, -np.inf, dtype)
        self.t1 = np.full(n, np.inf, dtype)
        self.face = np.zeros(n, np.int64)
        self.alive = np.ones(n, bool)

    def plane(self, denom, dist, k):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = dist / denom
        upd = (denom < 0) & (t > self.t0)
        self.face = np.where(upd, k, self.face)
        self.t0 = np.where(upd, t, self.t0)
        self.t1 = np.where((denom > 0) & (t < self.t1), t, self.t1)
        self.alive &= ~((denom == 0) & (dist < 0))

    def hit(self):
        return self.alive & (self.t0 > 0) & (self.t0 <= self.t1)


def _sphere_entry(o, d, a, c, r2):
    oc = o - c
    tc = -_dot(oc, d) / a
    q = oc + d * tc[:, None]
    q2 = _dot(q, q)
    ok = q2 <= r2
    with np.errstate(invalid="ignore"):
        t = tc - np.sqrt(np.where(ok, (r2 - q2) / a, 0))
    return np.where(ok, t, np.inf).astype(o.dtype)


def _cyl_interval(o, d, r2):
    """The infinite cylinder about z: (alive, t_in, t_out, a)"""
    dt = o.dtype
    a = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    pos = a > 0
    sa = np.where(pos, a, 1).astype(dt)
    tc = -(o[:, 0] * d[:, 0] + o[:, 1] * d[:, 1]) / sa
    qx, qy = o[:, 0] + tc * d[:, 0], o[:, 1] + tc * d[:, 1]
    q2 = qx * qx + qy * qy
    inside = q2 <= r2
    hh = np.sqrt(np.where(inside, (r2 - q2) / sa, 0)).astype(dt)
    par_in = ~pos & ~(o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1] > r2)
    alive = (pos & inside) | par_in
    t_in = np.where(pos, tc - hh, -np.inf).astype(dt)
    t_out = np.where(pos, tc + hh, np.inf).astype(dt)
    return alive, t_in, t_out, pos


def intersect(gtype, size, planes, o, d):
    """Rays (o, d) [N, 3] in the geom's frame -> (t [N], inf on a miss; outward normal [N, 3] in the geom's frame)."""
    dt = o.dtype
    n = len(o)
    inf = np.full(n, np.inf, dt)
    nrm = np.zeros((n, 3), dt)
    nrm[:, 2] = 1
    if gtype in (SPHERE, ELLIPSOID):
        os_, ds = o / size, d / size
        t = _sphere_entry(os_, ds, _dot(ds, ds), np.zeros(3, dt), dt.type(1))
        ok = np.isfinite(t) & (t > 0)
        h = (os_ + ds * np.where(ok, t, 0)[:, None]) / size
        with np.errstate(invalid="ignore", divide="ignore"):
            hn = h / np.sqrt(_dot(h, h))[:, None]
        return np.where(ok, t, inf), np.where(ok[:, None], hn, nrm).astype(dt)
    if gtype == CAPSULE:
        r, hl = size[0], size[1]
        r2 = r * r
        alive, t_in, _, pos = _cyl_interval(o, d, r2)
        z = o[:, 2] + np.where(pos, t_in, 0) * d[:, 2]
        side = pos & alive & (t_in > 0) & (np.abs(z) <= hl)
        best = np.where(side, t_in, inf)
        tt = np.where(side, t_in, 0)
        bn = np.where(side[:, None], np.stack([(o[:, 0] + tt * d[:, 0]) / r, (o[:, 1] + tt * d[:, 1]) / r, np.zeros(n, dt)], -1), nrm)
        dd = _dot(d, d)
        for sgn in (1, -1):
            c = np.array([0, 0, sgn * hl], dt)
            t = _sphere_entry(o, d, dd, c, r2)
            ok = np.isfinite(t) & (t > 0) & (t < best)
            tt = np.where(ok, t, 0)
            bn = np.where(ok[:, None], (o + d * tt[:, None] - c) / r, bn)
            best = np.where(ok, t, best)
        miss = pos & ~alive  # (outside the infinite cylinder: the caps lie inside it)
        return np.where(miss, inf, best).astype(dt), bn.astype(dt)
    if gtype == CYLINDER:
        r, hl = size[0], size[1]
        alive, t_in, t_out, _ = _cyl_interval(o, d, r * r)
        c = _Clip(n, dt)
        c.t0, c.t1, c.alive = t_in, t_out, alive
        c.plane(d[:, 2], hl - o[:, 2], 1)
        c.plane(-d[:, 2], hl + o[:, 2], 2)
        ok = c.hit()
        tt = np.where(ok, c.t0, 0)
        side = np.stack([(o[:, 0] + tt * d[:, 0]) / r, (o[:, 1] + tt * d[:, 1]) / r, np.zeros(n, dt)], -1)
        cap = np.stack([np.zeros(n, dt), np.zeros(n, dt), np.where(c.face == 1, 1, -1).astype(dt)], -1)
        return np.where(ok, c.t0, inf).astype(dt), np.where((c.face == 0)[:, None], side, cap).astype(dt)
    if gtype == BOX:
        c = _Clip(n, dt)
        for k in range(3):
            c.plane(d[:, k], size[k] - o[:, k], 2 * k)
            c.plane(-d[:, k], size[k] + o[:, k], 2 * k + 1)
        ok = c.hit()
        out = np.zeros((n, 3), dt)
        out[np.arange(n), c.face >> 1] = np.where(c.face & 1, -1, 1)
        return np.where(ok, c.t0, inf).astype(dt), out
    if gtype == MESH:
        c = _Clip(n, dt)
        for k, p in enumerate(planes):
            c.plane(p[0] * d[:, 0] + p[1] * d[:, 1] + p[2] * d[:, 2], p[3] - (p[0] * o[:, 0] + p[1] * o[:, 1] + p[2] * o[:, 2]), k)
        ok = c.hit()
        return np.where(ok, c.t0, inf).astype(dt), planes[c.face, :3].astype(dt)
    raise ValueError(f"geom type {gtype}")


def _cast(s, gp, gr, org, dirs, any_hit=False):
    """Nearest entry over all visuals (index order, strict <), then the ground plane.  org, dirs: [N, 3]; gp [ng, 3], gr [ng, 3, 3]."""
    dt = org.dtype
    n = len(org)
    best = np.full(n, np.inf, dt)
    gid = np.full(n, -1, np.int64)
    bn = np.zeros((n, 3), dt)
    bn[:, 2] = 1
    for g in range(s["ngeom"]):
        r = gr[g]
        ol = (org - gp[g]) @ r  # R^T (o - p)
        dl = dirs @ r
        a, cnt = s["geom_hull"][g]
        t, nl = intersect(int(s["geom_type"][g]), s["geom_size"][g], s["hull_plane"][a:a + cnt], ol.astype(dt), dl.astype(dt))
        upd = t < best
        best = np.where(upd, t, best)
        gid = np.where(upd, g, gid)
        bn = np.where(upd[:, None], (nl @ r.T).astype(dt), bn)
    if s["has_plane"] and not any_hit:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (dt.type(s["plane_z"]) - org[:, 2]) / dirs[:, 2]
        upd = (dirs[:, 2] != 0) & (t > 0) & (t < best)
        best = np.where(upd, t, best)
        gid = np.where(upd, s["ngeom"], gid)
        bn = np.where(upd[:, None], np.array([0, 0, 1], dt), bn)
    return best.astype(dt), gid, bn.astype(dt)


def trace(s, gp, gr, cam_pos, cam_rot, dirs_cam):
    """One frame.  -> dict(depth, geom_id, parity, shadow, rgb uint8, colour float) per ray."""
    dt = gp.dtype
    ty = dt.type
    n = len(dirs_cam)
    org = np.broadcast_to(cam_pos, (n, 3)).astype(dt)
    dirs = dirs_cam @ cam_rot.T
    dirs = (dirs / np.sqrt(_dot(dirs, dirs))[:, None]).astype(dt)
    depth, gid, bn = _cast(s, gp, gr, org, dirs)
    hitm = gid >= 0
    hit = org + dirs * np.where(hitm, depth, 0)[:, None]
    light = np.array(LIGHT, dt)
    ground = gid == s["ngeom"]
    parity = np.where(ground, (np.floor(hit[:, 0]).astype(np.int64) + np.floor(hit[:, 1]).astype(np.int64)) & 1, 0)
    base = np.where(parity[:, None] == 1, np.array(TONE_ODD, dt), np.array(TONE_EVEN, dt))
    if s["ngeom"]:
        base = np.where((hitm & ~ground)[:, None], s["geom_rgb"][np.clip(gid, 0, s["ngeom"] - 1)], base)
    lit = np.maximum(_dot(bn, light), 0).astype(dt)
    need = hitm & (lit > 0)
    shadow = np.zeros(n, bool)
    if need.any():
        so = (hit + bn * ty(SHADOW_BIAS))[need].astype(dt)
        ld = np.broadcast_to(light, so.shape).astype(dt)
        _, sid, _ = _cast(s, gp, gr, so, ld, any_hit=True)
        shadow[need] = sid >= 0
    lit = np.where(shadow, 0, lit).astype(dt)
    col = base * (ty(AMBIENT) + ty(DIFFUSE) * lit)[:, None]
    col = np.where(hitm[:, None], col, np.array(SKY, dt)).astype(dt)
    rgb = np.floor(np.clip(col, 0, 1) * ty(255) + ty(0.5)).astype(np.uint8)
    return dict(depth=np.where(hitm, depth, np.inf).astype(dt), geom_id=np.where(hitm, gid, -1), parity=parity, shadow=shadow, rgb=rgb)


def render(cm, qpos, camera, W, H, dtype=np.float64, tilt=(0.0, 0.0)):
    """All frames.  -> dict of [F, H, W(, 3)] arrays (depth, geom_id, parity, shadow, rgb) + geom_pose [F, ng, 12] + xpos."""
    dtype = np.dtype(dtype)
    s = scene_of(cm, dtype)
    gp, gr, cp, cr, xpos = poses(cm, s, qpos, camera, dtype)
    dc = camera_rays(s["cam_tanhalf"][camera], W, H, dtype, tilt)
    frames = [trace(s, gp[f], gr[f], cp[f], cr[f], dc) for f in range(len(gp))]
    out = {k: np.stack([fr[k] for fr in frames]).reshape((len(gp), H, W) + frames[0][k].shape[1:]) for k in frames[0]}
    out["geom_pose"] = np.concatenate([gp, gr.reshape(gr.shape[0], gr.shape[1], 9)], -1)
    out["xpos"] = xpos
    return out


def compared(cm, qpos, camera, W, H):
    """-> (the float64 oracle's render, mask [F, H, W] of the pixels whose key is the same under the four DELTA tilts)"""
    ref = render(cm, qpos, camera, W, H)
    key = lambda r: (r["geom_id"], r["parity"], r["shadow"])
    mask = np.ones(ref["geom_id"].shape, bool)
    for tilt in ((DELTA, 0.0), (-DELTA, 0.0), (0.0, DELTA), (0.0, -DELTA)):
        other = render(cm, qpos, camera, W, H, tilt=tilt)
        for a, b in zip(key(ref), key(other)):
            mask &= a == b
    return ref, mask
