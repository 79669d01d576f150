"""Rendering rollouts: the scene blob, `Renderer` / `render` over `mppo_render`, and `write_video`.

Stands where the reference calls `env.render(rollout[::render_every], camera=..., width=..., height=...)` (`minppo/env.py:264-333`, the
MuJoCo renderer behind Brax).  There is no MuJoCo here and none is needed: every shape the engine accepts - sphere, capsule, cylinder, box,
ellipsoid, convex hull, the ground plane - has a closed-form ray intersection, so frames are ray-cast on the device (csrc/k_render.hip).

  scene_blob(cm)            the little-endian blob `mppo_scene_open` reads (layout: csrc/render.h): dimensions, the kinematic tree taken from
                            `cm.t`, the visuals (`cm.visuals`: every geom of the MJCF, colliding or not, in document order; a built-in robot's
                            colliders in MuJoCo's default colour), hull faces as planes in the geom frame, the ground plane, the cameras
  Renderer(cm, lib=, xp=)   an open scene; `.render(qpos, camera, width, height)` -> uint8 [F, H, W, 3]
  render(cm, qpos, ...)     the same in one call
  write_video(path, frames, fps)   .npz, .avi (uncompressed, written here) or .mp4 (through an installed ffmpeg)

What is approximated: a mesh is drawn as its CONVEX HULL (what the engine collides it as); one sample per pixel (no anti-aliasing); no
textures; alpha is ignored except that a geom with alpha 0 is not drawn.  Cameras: `fixed` (rigid in its body's frame) and `track` (offset from
the body's position, orientation fixed in the world, both as they are at qpos0); every model has the camera `track` (model.compile_model).
"""

from __future__ import annotations

import ctypes as C
import logging
import math
import os
import shutil
import struct
import subprocess
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from minppo_amd import _native as nat
from minppo_amd.model import (GEOM_BOX, GEOM_CAPSULE, GEOM_CYLINDER, GEOM_ELLIPSOID, GEOM_MESH, GEOM_SPHERE, JNT_FREE, CompiledModel, _normalize, _qmat, _qmul)

logger = logging.getLogger(__name__)

SCENE_MAGIC = 0x4353504D  # "MPSC"
SCENE_VERSION = 1
SCENE_HEADER_WORDS = 16
MAX_VISUALS = 512  # csrc/render.h kSceneMaxGeoms: 24 words of LDS per visual
MAX_HULL_VERTS = 64  # a drawn hull keeps at most this many vertices (qhull's TA option, as a collision mesh's maxhullvert)
CAM_FIXED, CAM_TRACK, CAM_UNSUPPORTED = 0, 1, 2

# the arrays of the blob in directory order (csrc/render.h SceneArray)
_SCENE_INT = ["body_parent", "body_jntadr", "body_jntnum", "jnt_type", "jnt_qposadr", "geom_body", "geom_type", "geom_hull", "cam_body", "cam_mode"]
_SCENE_F32 = ["body_pos", "body_quat", "jnt_pos", "jnt_axis", "qpos0", "geom_size", "geom_pos", "geom_mat", "geom_rgb", "geom_rbound", "hull_plane", "cam_pos", "cam_mat",
              "cam_tanhalf"]


def hull_planes(points: Any) -> np.ndarray:
    """The faces of the convex hull of `points` as planes [F, 4]: outward unit normal and offset (n . x <= offset inside), coplanar
    triangles merged."""
    from minppo_amd.mjcf import convex_hull_vertices
    from minppo_amd.model import hull_topology

    pts = np.asarray(points, np.float64).reshape(-1, 3)
    try:
        verts = convex_hull_vertices(pts, "visual mesh")
    except ValueError:  # more hull vertices than a collider may have: capped the way a collision mesh's maxhullvert caps it (a degenerate mesh raises again)
        verts = convex_hull_vertices(pts, "visual mesh", MAX_HULL_VERTS)
    faces, normals, _, _ = hull_topology(verts)
    return np.concatenate([normals, [[float(np.dot(normals[k], verts[f[0]]))] for k, f in enumerate(faces)]], axis=1)


def _world_quats0(cm: CompiledModel) -> np.ndarray:
    """World orientation of every body at qpos0 (joint displacements are zero there; a free body's is its qpos0 quaternion)."""
    t = cm.t
    xq = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (cm.nbody, 1))
    for b in range(1, cm.nbody):
        q = _qmul(xq[t["body_parent"][b]], t["body_quat"][b])
        for j in range(t["body_jntadr"][b], t["body_jntadr"][b] + t["body_jntnum"][b]):
            if t["jnt_type"][j] == JNT_FREE:
                q = _normalize(t["qpos0"][t["jnt_qposadr"][j] + 3:t["jnt_qposadr"][j] + 7])
        xq[b] = _normalize(q)
    return xq


def camera_names(cm: CompiledModel) -> List[str]:
    return [c.name for c in cm.cameras]


def camera_index(cm: CompiledModel, name: str) -> int:
    """Index of the camera `name`; ValueError (listing the known names) for an unknown one, and for one whose mode is not drawn."""
    names = camera_names(cm)
    if name not in names:
        raise ValueError(f"unknown camera {name!r}: the model {cm.name!r} has the cameras {names}")
    cam = cm.cameras[names.index(name)]
    if cam.mode not in ("fixed", "track"):
        raise ValueError(f"camera {name!r} has mode={cam.mode!r}: the renderer draws fixed and track cameras only")
    return names.index(name)


def scene_arrays(cm: CompiledModel) -> Dict[str, np.ndarray]:
    """The scene as named arrays (float64 / int32): what `scene_blob` packs.  A visual that cannot be drawn - an unresolved mesh, a
    degenerate hull, alpha 0 - is left out; the unresolved ones with one warning each."""
    t = cm.t
    gbody, gtype, ghull, gsize, gpos, gmat, grgb, grb = [], [], [], [], [], [], [], []
    planes: List[np.ndarray] = []
    nface = 0
    for k, (body, v) in enumerate(cm.visuals):
        what = f"visual {k} of body {cm.body_names[body]!r}"
        if v.problem:
            logger.warning("%s is not drawn: %s", what, v.problem)
            continue
        if len(v.rgba) > 3 and float(v.rgba[3]) == 0.0:
            continue
        size = [float(x) for x in v.size]
        hull = (0, 0)
        if v.type == GEOM_SPHERE:
            size3, rb = [size[0]] * 3, size[0]
        elif v.type == GEOM_CAPSULE:
            size3, rb = [size[0], size[1], 0.0], size[0] + size[1]
        elif v.type == GEOM_CYLINDER:
            size3, rb = [size[0], size[1], 0.0], math.hypot(size[0], size[1])
        elif v.type in (GEOM_BOX, GEOM_ELLIPSOID):
            size3, rb = size[:3], (float(np.linalg.norm(size[:3])) if v.type == GEOM_BOX else max(size[:3]))
        elif v.type == GEOM_MESH:
            try:
                pl = hull_planes(v.vertices)
            except Exception as exc:  # noqa: BLE001 - qhull on a flat or empty point set
                logger.warning("%s is not drawn: its convex hull cannot be formed (%s)", what, str(exc).splitlines()[0] if str(exc) else type(exc).__name__)
                continue
            hull = (nface, len(pl))
            planes.append(pl)
            nface += len(pl)
            size3, rb = [0.0, 0.0, 0.0], float(np.linalg.norm(np.asarray(v.vertices, np.float64).reshape(-1, 3), axis=1).max())
        else:
            logger.warning("%s is not drawn: geom type %d", what, v.type)
            continue
        gbody.append(body); gtype.append(v.type); ghull.append(hull); gsize.append(size3); gpos.append([float(x) for x in v.pos])
        gmat.append(_qmat(_normalize(v.quat))); grgb.append([float(x) for x in v.rgba[:3]]); grb.append(rb)
    ng = len(gbody)
    xq0 = _world_quats0(cm)
    cbody, cmode, cpos, cmat, cth = [], [], [], [], []
    for c in cm.cameras:
        b = c.bodyid if c.bodyid >= 0 else 0
        mode = {"fixed": CAM_FIXED, "track": CAM_TRACK}.get(c.mode, CAM_UNSUPPORTED)
        pos, mat = np.asarray(c.pos, np.float64), _qmat(_normalize(c.quat))
        if mode == CAM_TRACK:  # the offset and the orientation in the WORLD frame, as they are at qpos0
            r0 = _qmat(xq0[b])
            pos, mat = r0 @ pos, r0 @ mat
        fovy = float(c.fovy)
        if not 0.0 < fovy < 180.0:
            mode, fovy = CAM_UNSUPPORTED, 45.0
        cbody.append(b); cmode.append(mode); cpos.append(pos); cmat.append(mat); cth.append(math.tan(math.radians(fovy) / 2))
    i32 = lambda a, shape: np.asarray(a, np.int32).reshape(shape)
    f64 = lambda a, shape: np.asarray(a, np.float64).reshape(shape)
    return dict(
        nq=cm.nq, nbody=cm.nbody, njnt=cm.njnt, ngeom=ng, ncam=len(cm.cameras), has_plane=int(bool(cm.has_plane)), plane_z=float(t["plane_z"]), nface=nface,
        body_parent=i32(t["body_parent"], -1), body_jntadr=i32(t["body_jntadr"], -1), body_jntnum=i32(t["body_jntnum"], -1), jnt_type=i32(t["jnt_type"], -1),
        jnt_qposadr=i32(t["jnt_qposadr"], -1), geom_body=i32(gbody, -1), geom_type=i32(gtype, -1), geom_hull=i32(ghull, (ng, 2)), cam_body=i32(cbody, -1), cam_mode=i32(cmode, -1),
        body_pos=f64(t["body_pos"], (-1, 3)), body_quat=f64(t["body_quat"], (-1, 4)), jnt_pos=f64(t["jnt_pos"], (-1, 3)), jnt_axis=f64(t["jnt_axis"], (-1, 3)), qpos0=f64(t["qpos0"], -1),
        geom_size=f64(gsize, (ng, 3)), geom_pos=f64(gpos, (ng, 3)), geom_mat=f64(gmat, (ng, 3, 3)), geom_rgb=f64(grgb, (ng, 3)), geom_rbound=f64(grb, -1),
        hull_plane=f64(np.concatenate(planes) if planes else [], (nface, 4)), cam_pos=f64(cpos, (-1, 3)), cam_mat=f64(cmat, (-1, 3, 3)), cam_tanhalf=f64(cth, -1))


def pack_scene(s: Dict[str, Any]) -> bytes:
    """`scene_arrays` -> the blob: 16 header words, the (offset, count) directory, the arrays, each padded to 4 words."""
    names = _SCENE_INT + _SCENE_F32
    cursor = (SCENE_HEADER_WORDS + 2 * len(names) + 3) // 4 * 4
    base = cursor
    payload, directory = bytearray(), bytearray()
    for k in names:
        a = np.ascontiguousarray(s[k]).reshape(-1)
        raw = a.astype("<i4" if k in _SCENE_INT else "<f4").tobytes()
        directory += struct.pack("<2i", cursor, a.size)
        pad = (-a.size) % 4
        payload += raw + b"\0" * (4 * pad)
        cursor += a.size + pad
    hdr = bytearray(4 * SCENE_HEADER_WORDS)
    struct.pack_into("<3I6i", hdr, 0, SCENE_MAGIC, SCENE_VERSION, cursor, s["nq"], s["nbody"], s["njnt"], s["ngeom"], s["ncam"], s["has_plane"])
    struct.pack_into("<f2i", hdr, 36, s["plane_z"], s["nface"], len(names))
    directory += b"\0" * (4 * (base - SCENE_HEADER_WORDS - 2 * len(names)))
    blob = bytes(hdr) + bytes(directory) + bytes(payload)
    assert len(blob) == 4 * cursor
    return blob


def scene_blob(cm: CompiledModel) -> bytes:
    s = scene_arrays(cm)
    if s["ngeom"] > MAX_VISUALS:
        raise ValueError(f"model {cm.name!r} has {s['ngeom']} visuals: the renderer draws at most {MAX_VISUALS}")
    return pack_scene(s)


class Renderer:
    """An open scene of one compiled model.  `lib=` / `xp="numpy"` as in `Trainer` and `evaluate`: the default is the HIP library with
    torch tensors as device memory; the test-suite's emulator build runs with NumPy arrays."""

    def __init__(self, cm: CompiledModel, *, lib: Optional[nat.Lib] = None, xp: str = "torch", device: Any = "cuda:0") -> None:
        self.cm = cm
        self.lib = lib if lib is not None else nat.load()
        self.xp = xp
        self._host = np.frombuffer(scene_blob(cm), np.uint8).copy()
        self._scene = C.c_void_p()
        if xp == "torch":
            import torch

            self.torch = torch
            self.device = torch.device(device)
            self._dev = torch.from_numpy(self._host.copy()).to(self.device)
            with torch.cuda.device(self.device):
                self.lib.scene_open(self._host.ctypes.data, self._host.size, self._dev.data_ptr(), C.byref(self._scene))
        else:
            self.torch, self.device = None, None
            self._dev = self._host.copy()
            self.lib.scene_open(self._host.ctypes.data, self._host.size, self._dev.ctypes.data, C.byref(self._scene))
        self.dims = nat.SceneDims()
        self.lib.scene_get_dims(self._scene, C.byref(self.dims))

    def render_raw(self, qpos: Any, camera: str = "track", width: int = 640, height: int = 480, outputs: Sequence[str] = ("rgb",)) -> Dict[str, np.ndarray]:
        """`qpos`: [F, q_ld] with q_ld >= nq (joint positions, state records or trajectory rows: qpos leads each), a torch tensor on the
        scene's device or anything NumPy reads.  -> the requested outputs of `mppo_render` (rgb, depth, geom_id, geom_pose) as host arrays."""
        if not self._scene:
            raise RuntimeError("the renderer is closed")
        cam = camera_index(self.cm, camera)
        unknown = set(outputs) - {"rgb", "depth", "geom_id", "geom_pose"}
        if unknown:
            raise ValueError(f"unknown render output(s) {sorted(unknown)}")
        W, H, ng = int(width), int(height), self.dims.ngeom
        if W < 1 or H < 1:
            raise ValueError(f"image size {W} x {H}")
        torch = self.torch
        if torch is not None:
            q = qpos if hasattr(qpos, "data_ptr") else torch.from_numpy(np.ascontiguousarray(np.asarray(qpos, np.float32)))
            q = q.to(device=self.device, dtype=torch.float32).contiguous()
        else:
            q = np.ascontiguousarray(np.asarray(qpos.detach().cpu().numpy() if hasattr(qpos, "detach") else qpos, np.float32))
        if q.ndim != 2 or q.shape[1] < self.cm.nq:
            raise ValueError(f"qpos must be [F, >= {self.cm.nq}], got {tuple(q.shape)}")
        F, q_ld = int(q.shape[0]), int(q.shape[1])
        if F == 0:
            raise ValueError("no frames to render")
        shapes = dict(rgb=((F, H, W, 3), "uint8"), depth=((F, H, W), "float32"), geom_id=((F, H, W), "int32"), geom_pose=((F, ng, 12), "float32"))
        bufs: Dict[str, Any] = {}
        for k in outputs:
            shape, dt = shapes[k]
            bufs[k] = torch.zeros(shape, dtype=getattr(torch, dt), device=self.device) if torch is not None else np.zeros(shape, dt)
        out = nat.RenderOut(**{k: nat.ptr(v) for k, v in bufs.items()})
        if torch is not None:
            with torch.cuda.device(self.device):
                stream = torch.cuda.current_stream(self.device)
                self.lib.render(self._scene, F, q.data_ptr(), q_ld, cam, W, H, C.byref(out), stream.cuda_stream)
                stream.synchronize()
            return {k: v.cpu().numpy() for k, v in bufs.items()}
        self.lib.render(self._scene, F, q.ctypes.data, q_ld, cam, W, H, C.byref(out), None)
        return bufs

    def render(self, qpos: Any, camera: str = "track", width: int = 640, height: int = 480) -> np.ndarray:
        return self.render_raw(qpos, camera, width, height)["rgb"]

    def close(self) -> None:
        if getattr(self, "_scene", None):
            if self.torch is not None:
                self.torch.cuda.synchronize(self.device)
            self.lib.scene_close(self._scene)
            self._scene = None

    def __enter__(self) -> "Renderer":
        return self

    def __exit__(self, *exc: Any) -> None:
        self.close()


def render(cm: CompiledModel, qpos: Any, camera: str = "track", width: int = 640, height: int = 480, *, lib: Optional[nat.Lib] = None, xp: str = "torch",
           device: Any = "cuda:0") -> np.ndarray:
    """Frames [F, H, W, 3] uint8 of the joint positions `qpos` [F, >= nq] of the model `cm`, seen by its camera `camera`."""
    with Renderer(cm, lib=lib, xp=xp, device=device) as r:
        return r.render(qpos, camera, width, height)


# ---------------------------------------------------------------------------------------------------------------------------------------
# video files
# ---------------------------------------------------------------------------------------------------------------------------------------


def _avi_bytes(frames: np.ndarray, fps: float) -> bytes:
    """An uncompressed RGB24 AVI (RIFF): bottom-up BGR rows padded to four bytes, one `00db` chunk per frame, an `idx1` index."""
    F, H, W, _ = frames.shape
    stride = (3 * W + 3) & ~3
    fsize = stride * H
    scale, rate = 1000, max(1, int(round(float(fps) * 1000)))
    chunks, index, off = bytearray(), bytearray(), 4
    for f in range(F):
        rows = np.zeros((H, stride), np.uint8)
        rows[:, :3 * W] = frames[f, ::-1, :, ::-1].reshape(H, 3 * W)
        chunks += b"00db" + struct.pack("<I", fsize) + rows.tobytes()
        index += b"00db" + struct.pack("<3I", 0x10, off, fsize)
        off += 8 + fsize
    avih = struct.pack("<14I", int(round(1e6 / (rate / scale))), int(fsize * rate / scale), 0, 0x10, F, 0, 1, fsize, W, H, 0, 0, 0, 0)
    strh = b"vids" + b"DIB " + struct.pack("<I2H8I4h", 0, 0, 0, 0, scale, rate, 0, F, fsize, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf = struct.pack("<3i2H6i", 40, W, H, 1, 24, 0, fsize, 0, 0, 0, 0)
    chunk = lambda tag, data: tag + struct.pack("<I", len(data)) + data
    lst = lambda tag, data: b"LIST" + struct.pack("<I", 4 + len(data)) + tag + data
    body = b"AVI " + lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf))) + lst(b"movi", bytes(chunks)) + chunk(b"idx1", bytes(index))
    return b"RIFF" + struct.pack("<I", len(body)) + body


def write_video(path: Any, frames: Any, fps: float) -> None:
    """Writes uint8 frames [F, H, W, 3] by the extension of `path`: .npz (`frames`, `fps`), .avi (uncompressed RGB24, written here: needs
    nothing installed) or .mp4 (raw frames piped to `ffmpeg`, when one is installed)."""
    frames = np.ascontiguousarray(np.asarray(frames))
    if frames.ndim != 4 or frames.shape[-1] != 3 or frames.dtype != np.uint8:
        raise ValueError(f"write_video: frames must be uint8 [F, H, W, 3], got {frames.dtype} {frames.shape}")
    path = os.fspath(path)
    ext = os.path.splitext(path)[1].lower()
    if ext not in (".npz", ".avi", ".mp4"):
        raise ValueError(f"write_video: {path!r} - .npz, .avi or .mp4")
    if ext == ".mp4" and shutil.which("ffmpeg") is None:
        raise ImportError("`ffmpeg` command not found. Please install it to save an .mp4 (an .avi or .npz needs nothing installed).")
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    if ext == ".npz":
        with open(path, "wb") as f:
            np.savez(f, frames=frames, fps=np.float64(fps))
    elif ext == ".avi":
        with open(path, "wb") as f:
            f.write(_avi_bytes(frames, fps))
    else:
        F, H, W, _ = frames.shape
        cmd = ["ffmpeg", "-y", "-loglevel", "error", "-f", "rawvideo", "-pix_fmt", "rgb24", "-s", f"{W}x{H}", "-r", str(fps), "-i", "-", "-an", "-pix_fmt", "yuv420p", path]
        r = subprocess.run(cmd, input=frames.tobytes(), capture_output=True)
        if r.returncode != 0:
            raise RuntimeError(f"ffmpeg failed writing {path!r}: {r.stderr.decode('utf-8', 'replace')[-500:]}")
