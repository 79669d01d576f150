// render.hip - mppo_scene_open / mppo_render: the host side of the renderer (kernels: k_render.hip).  What the reference leaves to MuJoCo's renderer
// (`env.render(rollout, camera, width, height)`, minppo/env.py:264-333): frames of a rollout as images, here ray-cast from the scene blob of
// minppo_amd/render.py - every shape the engine accepts has a closed-form ray intersection.
//
// parse_scene_blob is all there is between bytes that come from outside the program and kernels that follow the blob's indices (model_blob.hip does
// the same for the model blob): sizes and addresses in range, parents before children, body ids / types / hull ranges valid, every number finite,
// at most kSceneMaxGeoms visuals (their staged form must fit in LDS: more is an error, not a truncation).
//
// mppo_render makes two launches on the caller's stream.  The poses' scratch lives inside the handle and grows on demand.
#include "render.h"

#include <cmath>
#include <cstring>

#include "mppo_common.h"

namespace mppo {

static int scene_array_len(const SceneView& v, int k) {
  switch (k) {
    case SI_body_parent: case SI_body_jntadr: case SI_body_jntnum: return v.nbody;
    case SI_jnt_type: case SI_jnt_qposadr: return v.njnt;
    case SI_geom_body: case SI_geom_type: case SF_geom_rbound: return v.ngeom;
    case SI_geom_hull: return 2 * v.ngeom;
    case SI_cam_body: case SI_cam_mode: case SF_cam_tanhalf: return v.ncam;
    case SF_body_pos: return 3 * v.nbody;
    case SF_body_quat: return 4 * v.nbody;
    case SF_jnt_pos: case SF_jnt_axis: return 3 * v.njnt;
    case SF_qpos0: return v.nq;
    case SF_geom_size: case SF_geom_pos: case SF_geom_rgb: return 3 * v.ngeom;
    case SF_geom_mat: return 9 * v.ngeom;
    case SF_hull_plane: return 4 * v.nface;
    case SF_cam_pos: return 3 * v.ncam;
    case SF_cam_mat: return 9 * v.ncam;
    default: return -1;
  }
}

int32_t parse_scene_blob(const void* host_blob, size_t nbytes, SceneView* view) {
  SceneView& v = *view;
  v = SceneView{};
  if (nbytes < 4 * (size_t)(kSceneHeaderWords + 2 * SCENE_ARRAY_COUNT) || (nbytes & 3)) return fail(MPPO_EMODEL, "scene blob too small or not word-sized (%zu bytes)", nbytes);
  const uint32_t* w = static_cast<const uint32_t*>(host_blob);
  const int32_t* wi = static_cast<const int32_t*>(host_blob);
  const float* wf = static_cast<const float*>(host_blob);
  auto bad = [&](const char* what) { return fail(MPPO_EMODEL, "scene blob: %s", what); };
  if (w[0] != kSceneMagic) return fail(MPPO_EMODEL, "bad scene blob magic 0x%08x", w[0]);
  if (w[1] != kSceneVersion) return fail(MPPO_EMODEL, "unsupported scene blob version %u", w[1]);
  const size_t total = w[2];
  if (total * 4 != nbytes) return fail(MPPO_EMODEL, "scene blob size mismatch: header says %zu words, got %zu bytes", total, nbytes);
  if (wi[11] != SCENE_ARRAY_COUNT) return fail(MPPO_EMODEL, "scene blob has %d arrays, engine expects %d", wi[11], (int)SCENE_ARRAY_COUNT);
  v.nq = wi[3]; v.nbody = wi[4]; v.njnt = wi[5]; v.ngeom = wi[6]; v.ncam = wi[7]; v.has_plane = wi[8]; v.plane_z = wf[9]; v.nface = wi[10];
  if (v.ngeom > kSceneMaxGeoms) return fail(MPPO_EMODEL, "scene blob: %d visuals, the renderer stages at most %d in LDS", v.ngeom, kSceneMaxGeoms);
  if (v.nq < 1 || v.nq > 256 || v.nbody < 1 || v.nbody > 128 || v.njnt < 0 || v.njnt > 256 || v.ngeom < 0 || v.ncam < 1 || v.ncam > 64 || v.nface < 0 || v.nface > (1 << 16) ||
      (v.has_plane != 0 && v.has_plane != 1))
    return bad("dimension out of the supported range (nq <= 256, nbody <= 128, njnt <= 256, 1 .. 64 cameras, 65536 hull faces)");
  const int32_t* dir = wi + kSceneHeaderWords;
  const size_t dir_end = kSceneHeaderWords + 2 * (size_t)SCENE_ARRAY_COUNT;
  for (int k = 0; k < SCENE_ARRAY_COUNT; ++k) {
    const long off = dir[2 * k], cnt = dir[2 * k + 1];
    if (off < (long)dir_end || cnt < 0 || (size_t)off + (size_t)cnt > total || (off & 3)) return bad("array directory entry out of range");
    if (cnt != scene_array_len(v, k)) return fail(MPPO_EMODEL, "scene blob: array %d has %ld entries, expected %d", k, cnt, scene_array_len(v, k));
    v.o[k] = (int)off;
  }
  auto fin = [](float x) { return x == x && x - x == 0.f; };
  if (!fin(v.plane_z)) return bad("plane_z is not finite");
  for (int k = kSceneFirstFloat; k < SCENE_ARRAY_COUNT; ++k)
    for (int i = 0, n = dir[2 * k + 1]; i < n; ++i)
      if (!fin(wf[v.o[k] + i])) return fail(MPPO_EMODEL, "scene blob: array %d holds a value that is not finite (entry %d)", k, i);
  const int32_t *par = wi + v.o[SI_body_parent], *ja = wi + v.o[SI_body_jntadr], *jn = wi + v.o[SI_body_jntnum], *jt = wi + v.o[SI_jnt_type], *qa = wi + v.o[SI_jnt_qposadr];
  if (par[0] != 0) return bad("the world's parent must be the world");
  for (int b = 1; b < v.nbody; ++b) {
    if (par[b] < 0 || par[b] >= b) return fail(MPPO_EMODEL, "scene blob: body %d has parent %d: bodies are not topologically ordered", b, par[b]);
    if (jn[b] < 0 || (jn[b] > 0 && (ja[b] < 0 || ja[b] + jn[b] > v.njnt))) return bad("body joint range out of bounds");
  }
  if (jn[0] != 0) return bad("the world has no joints");
  for (int j = 0; j < v.njnt; ++j) {
    const int width = jt[j] == 0 ? 7 : jt[j] == 1 ? 4 : 1;
    if (jt[j] < 0 || jt[j] > 3) return bad("unsupported joint type");
    if (qa[j] < 0 || qa[j] + width > v.nq) return bad("joint qpos address out of range");
  }
  const int32_t *gb = wi + v.o[SI_geom_body], *gt = wi + v.o[SI_geom_type], *gh = wi + v.o[SI_geom_hull];
  const float* gs = wf + v.o[SF_geom_size];
  for (int g = 0; g < v.ngeom; ++g) {
    if (gb[g] < 0 || gb[g] >= v.nbody) return fail(MPPO_EMODEL, "scene blob: visual %d names body %d of %d", g, gb[g], v.nbody);
    const float* s = gs + 3 * g;
    switch (gt[g]) {
      case RG_SPHERE: case RG_ELLIPSOID: case RG_BOX:
        if (!(s[0] > 0.f && s[1] > 0.f && s[2] > 0.f)) return fail(MPPO_EMODEL, "scene blob: visual %d needs three positive sizes", g);
        break;
      case RG_CAPSULE:
        if (!(s[0] > 0.f && s[1] >= 0.f)) return fail(MPPO_EMODEL, "scene blob: capsule %d needs a positive radius and a half length >= 0", g);
        break;
      case RG_CYLINDER:
        if (!(s[0] > 0.f && s[1] > 0.f)) return fail(MPPO_EMODEL, "scene blob: cylinder %d needs a positive radius and half length", g);
        break;
      case RG_MESH:
        if (gh[2 * g] < 0 || gh[2 * g + 1] < 4 || (long)gh[2 * g] + gh[2 * g + 1] > v.nface)
          return fail(MPPO_EMODEL, "scene blob: visual %d: hull faces %d + %d past the end of %d", g, gh[2 * g], gh[2 * g + 1], v.nface);
        break;
      default:
        return fail(MPPO_EMODEL, "scene blob: visual %d has geom type %d", g, gt[g]);
    }
  }
  const int32_t *cb = wi + v.o[SI_cam_body], *cmode = wi + v.o[SI_cam_mode];
  const float* cth = wf + v.o[SF_cam_tanhalf];
  for (int c = 0; c < v.ncam; ++c) {
    if (cb[c] < 0 || cb[c] >= v.nbody) return bad("camera body out of range");
    if (cmode[c] < CAM_FIXED || cmode[c] > CAM_UNSUPPORTED) return bad("camera mode out of range");
    if (!(cth[c] > 0.f)) return bad("a camera's field of view must be inside (0, 180) degrees");
  }
  return MPPO_OK;
}

}  // namespace mppo

using namespace mppo;

struct mppo_scene {
  SceneView view;
  const void* dev_blob;
  float* scratch;
  size_t scratch_bytes;
  int32_t cam_mode[64];  // (host copy: a camera whose mode the kernels do not draw is refused before anything is launched)
};

extern "C" int32_t mppo_scene_open(const void* host_blob, size_t nbytes, const void* dev_blob, mppo_scene_t** out) {
  MPPO_REQUIRE(host_blob && dev_blob && out, "mppo_scene_open: null blob / out");
  MPPO_REQUIRE((reinterpret_cast<uintptr_t>(host_blob) & 3) == 0 && (reinterpret_cast<uintptr_t>(dev_blob) & 3) == 0, "mppo_scene_open: the blobs must be 4-byte aligned");
  SceneView v;
  MPPO_TRY(parse_scene_blob(host_blob, nbytes, &v));
  mppo_scene* s = new mppo_scene();
  s->view = v;
  s->dev_blob = dev_blob;
  s->scratch = nullptr;
  s->scratch_bytes = 0;
  memcpy(s->cam_mode, static_cast<const int32_t*>(host_blob) + v.o[SI_cam_mode], sizeof(int32_t) * (size_t)v.ncam);
  *out = s;
  return MPPO_OK;
}

extern "C" int32_t mppo_scene_close(mppo_scene_t* s) {
  if (!s) return MPPO_OK;
  if (s->scratch) (void)hipFree(s->scratch);
  delete s;
  return MPPO_OK;
}

extern "C" int32_t mppo_scene_get_dims(const mppo_scene_t* s, mppo_scene_dims_t* out) {
  MPPO_REQUIRE(s && out, "mppo_scene_get_dims: null scene / out");
  out->nq = s->view.nq; out->nbody = s->view.nbody; out->ngeom = s->view.ngeom; out->ncam = s->view.ncam; out->has_plane = s->view.has_plane;
  return MPPO_OK;
}

extern "C" int32_t mppo_render(const mppo_scene_t* s, int32_t F, const float* qpos, int32_t q_ld, int32_t camera, int32_t width, int32_t height, const mppo_render_out_t* out,
                               void* stream) {
  MPPO_REQUIRE(s && qpos && out, "mppo_render: null scene / qpos / out");
  const SceneView& v = s->view;
  MPPO_REQUIRE(F >= 1 && F <= (1 << 20), "mppo_render: F = %d frames", F);
  MPPO_REQUIRE(q_ld >= v.nq, "mppo_render: q_ld = %d is less than nq = %d", q_ld, v.nq);
  MPPO_REQUIRE(camera >= 0 && camera < v.ncam, "mppo_render: camera %d of %d", camera, v.ncam);
  MPPO_REQUIRE(width >= 1 && width <= 8192 && height >= 1 && height <= 8192, "mppo_render: image %d x %d (1 .. 8192 each way)", width, height);
  MPPO_REQUIRE(s->cam_mode[camera] != CAM_UNSUPPORTED, "mppo_render: camera %d has a mode other than fixed / track", camera);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // scratch: body poses [F][nbody][7], camera [F][16], and the visuals' poses [F][ngeom][12] unless the caller wants them
  const size_t n_body = (size_t)F * v.nbody * 7, n_cam = (size_t)F * kCamWords, n_pose = out->geom_pose ? 0 : (size_t)F * v.ngeom * 12;
  const size_t need = (n_body + n_cam + n_pose) * sizeof(float);
  mppo_scene* ms = const_cast<mppo_scene*>(s);  // (the scratch is the handle's own: one render at a time per handle)
  if (need > ms->scratch_bytes) {
    if (ms->scratch) MPPO_CHECK_HIP(hipFree(ms->scratch));  // (synchronises with whatever still reads it)
    ms->scratch = nullptr;
    ms->scratch_bytes = 0;
    void* p = nullptr;
    MPPO_CHECK_HIP(hipMalloc(&p, need));
    ms->scratch = static_cast<float*>(p);
    ms->scratch_bytes = need;
  }
  float* body_ws = ms->scratch;
  float* camw = body_ws + n_body;
  float* pose = out->geom_pose ? out->geom_pose : camw + n_cam;
  MPPO_TRY(render_poses_launch(v, s->dev_blob, F, qpos, q_ld, camera, body_ws, pose, camw, st));
  if (!out->rgb && !out->depth && !out->geom_id) return MPPO_OK;
  return render_rays_launch(v, s->dev_blob, F, width, height, pose, camw, out->rgb, out->depth, out->geom_id, st);
}
