// model_blob.hip - the model blob's validator (model_view.h parse_model_blob): host arithmetic on bytes that come from outside the program, and all there is between
// them and a kernel that follows the blob's indices.  No HIP call, no kernel, no handle: tests/emu/blob_check_main.cpp links it alone, under the host sanitizers.
#include "model_view.h"
#include "mppo_common.h"

#include <initializer_list>

namespace mppo {

int32_t parse_model_blob(const void* host_blob, size_t nbytes, ModelView* view, BlobDims* dims, int* canon_words) {
  ModelView& v = *view;
  v = ModelView{};
  if (nbytes < 4 * (size_t)kBlobHeaderWords || (nbytes & 3)) return fail(MPPO_EMODEL, "model blob too small or not word-sized (%zu bytes)", nbytes);
  const uint32_t* w = static_cast<const uint32_t*>(host_blob);
  const int32_t* wi = static_cast<const int32_t*>(host_blob);
  const float* wf = static_cast<const float*>(host_blob);
  if (w[0] != kBlobMagic) return fail(MPPO_EMODEL, "bad model blob magic 0x%08x", w[0]);
  if (w[1] != kBlobVersion) return fail(MPPO_EMODEL, "unsupported model blob version %u", w[1]);
  const size_t total = w[2], hull_words = w[35];  // table part + hull section (+ the contact-parameter section: below, once the dims are known)
  if (wi[37] != 0 && wi[37] != 1) return fail(MPPO_EMODEL, "model blob: header word 37 (per-row contact parameters) is %d, not 0 or 1", wi[37]);
  if (wi[38] < 0 || wi[38] > kMaxEqRows) return fail(MPPO_EMODEL, "model blob: header word 38 (equality rows) is %d, not in [0, %d]", wi[38], kMaxEqRows);
  if ((total + hull_words) * 4 > nbytes || (wi[37] == 0 && wi[38] == 0 && (total + hull_words) * 4 != nbytes))
    return fail(MPPO_EMODEL, "model blob size mismatch: header says %zu + %zu words, got %zu bytes", total, hull_words, nbytes);
  if (wi[32] != BLOB_ARRAY_COUNT) return fail(MPPO_EMODEL, "model blob has %d arrays, engine expects %d", wi[32], (int)BLOB_ARRAY_COUNT);
  v.nq = wi[3]; v.nv = wi[4]; v.nu = wi[5]; v.nbody = wi[6]; v.njnt = wi[7]; v.ncon = wi[8]; v.nlimit = wi[9];
  v.iterations = wi[10]; v.ls_iterations = wi[11]; v.nlevel = wi[12]; v.nroot = wi[13]; v.include_c = wi[14] ? 1 : 0; v.npair = wi[15];
  v.ncvx = wi[33]; v.ncvxvert = wi[34];
  // every header dimension inside a bound that keeps the size arithmetic below (and in blob_offsets) far from overflow, BEFORE any of it
  // is computed (tests/test_blob_fuzz.py under UBSan: a dimension of INT_MAX overflowed `4 * ncon` here)
  for (int d : {v.nq, v.nv, v.nu, v.nbody, v.njnt, v.ncon, v.nlimit, v.iterations, v.ls_iterations, v.nlevel, v.nroot, v.npair, v.ncvx, v.ncvxvert, wi[36]})
    if (d < 0 || d > (1 << 16)) return fail(MPPO_EMODEL, "model blob: header dimension %d out of range", d);
  v.neq = wi[38];
  v.nefc = nefc_of(blob_dims_of(v));
  v.cparam = wi[37];
  const CParamView cpv = cparam_view(v.ncon, v.nlimit, v.ncvx);
  // the equality section behind it: its element count is its first word (read only once the words before it are known to exist)
  const size_t eq_at = total + hull_words + (v.cparam ? (size_t)cpv.words : 0);
  int eq_nel = 0;
  if (v.neq > 0) {
    if ((eq_at + 4) * 4 > nbytes) return fail(MPPO_EMODEL, "model blob size mismatch: no room for the equality section");
    eq_nel = wi[eq_at];
    if (eq_nel < 1 || eq_nel > v.neq) return fail(MPPO_EMODEL, "model blob: equality section holds %d elements for %d rows", eq_nel, v.neq);
    const EqView ev = eq_view(v.neq, eq_nel);
    if ((eq_at + (size_t)ev.words) * 4 != nbytes)
      return fail(MPPO_EMODEL, "model blob size mismatch: header says %zu + %d words (equality section), got %zu bytes", eq_at, ev.words, nbytes);
  }
  if (v.neq == 0 && v.cparam && (total + hull_words + (size_t)cpv.words) * 4 != nbytes)
    return fail(MPPO_EMODEL, "model blob size mismatch: header says %zu + %zu + %d words (contact-parameter section), got %zu bytes", total, hull_words, cpv.words, nbytes);
  v.timestep = wf[16]; v.tolerance = wf[17]; v.ls_tolerance = wf[18]; v.impratio = wf[19]; v.plane_z = wf[20]; v.meaninertia = wf[21];
  auto bad = [&](const char* what) { return fail(MPPO_EMODEL, "model blob: %s", what); };
  if (v.nq < 1 || v.nv < 1 || v.nbody < 2 || v.nbody > 128 || v.nv > 128 || v.nq > 256 || v.nu < 0 || v.nu > v.nv || v.njnt < 1 ||
      v.ncon < 0 || v.npair < 0 || v.npair > v.ncon || v.nlimit < 0 || v.nroot < 1 || v.nlevel < 1 || v.iterations < 0 || v.ls_iterations < 0 ||
      v.ncvx < 0 || 4 * v.ncvx > v.ncon - v.npair || v.ncvxvert < 4 * v.ncvx || v.ncvxvert > 64 * 64)
    return bad("dimension out of the supported range (nbody<=128, nv<=128, nq<=256)");
  if (!(v.timestep > 0.f) || !(v.meaninertia > 0.f) || !(v.impratio > 0.f)) return bad("non-positive timestep / meaninertia / impratio");
  const int32_t* dir = wi + kBlobHeaderWords;
  const BlobDims bd = blob_dims_of(v);  // (the table part follows from the dims read so far; cylinders, hull section and ball joints are counted below)
  const BlobOffsets canon = blob_offsets(bd);
  const size_t dir_end = kBlobHeaderWords + 2 * (size_t)BLOB_ARRAY_COUNT;
  if (dir_end > total) return bad("directory past the end");
  for (int k = 0; k < BLOB_ARRAY_COUNT; ++k) {
    const long off = dir[2 * k], cnt = dir[2 * k + 1];
    if (off < (long)dir_end || cnt < 0 || (size_t)(off + cnt) > total || (off & 3)) return bad("array directory entry out of range");
    if (cnt != blob_array_len(bd, k)) return fail(MPPO_EMODEL, "model blob: array %d has %ld entries, expected %d", k, cnt, blob_array_len(bd, k));
    if (off != canon.o[k]) return fail(MPPO_EMODEL, "model blob: array %d sits at word %ld, canonical placement is %d", k, off, canon.o[k]);
  }
  auto HI = [&](int k) { return wi + dir[2 * k]; };
  // index tables are validated here so that the kernel never dereferences out of range
  auto in_range = [&](int k, long lo, long hi_excl) {
    const int32_t* p = HI(k);
    for (long i = 0; i < dir[2 * k + 1]; ++i) if (p[i] < lo || p[i] >= hi_excl) return false;
    return true;
  };
  if (!in_range(BI_body_parent, 0, v.nbody) || !in_range(BI_body_rootid, 0, v.nbody) || !in_range(BI_jnt_bodyid, 1, v.nbody) ||
      !in_range(BI_jnt_qposadr, 0, v.nq) || !in_range(BI_jnt_dofadr, 0, v.nv) || !in_range(BI_dof_bodyid, 1, v.nbody) ||
      !in_range(BI_dof_jntid, 0, v.njnt) || !in_range(BI_dof_parentid, -1, v.nv) || !in_range(BI_dof_qposadr, -1, v.nq) ||
      !in_range(BI_act_dofid, 0, v.nv) || !in_range(BI_act_qposadr, 0, v.nq) || !in_range(BI_con_bodyid, 1, v.nbody) || !in_range(BI_pair_body, 1, v.nbody) ||
      !in_range(BI_lim_jntid, 0, v.njnt) || !in_range(BI_level_adr, 0, v.nbody) || !in_range(BI_level_body, 1, v.nbody) ||
      !in_range(BI_root_body, 1, v.nbody) || !in_range(BI_body_jntnum, 0, v.njnt + 1) || !in_range(BI_body_jntadr, -1, v.njnt) ||
      !in_range(BI_con_cvx, -4, 4 * v.ncvx) || !in_range(BI_cvx_body, 1, v.nbody) || !in_range(BI_cvx_vadr, 0, v.ncvxvert + 1))
    return bad("index table entry out of range");
  {
    const int32_t* va = HI(BI_cvx_vadr);
    for (int k = 0; k < v.ncvx; ++k) if (va[k + 1] < va[k] + 4 || va[k + 1] - va[k] > 64) return bad("a convex geom needs 4 .. 64 hull vertices");
    if (v.ncvx > 0 && (va[0] != 0 || va[v.ncvx] != v.ncvxvert)) return bad("cvx_vadr does not cover the vertex table");
    // cylinders: slots -2, -3, -4 in a row among the ground contacts, a half-axis vector of non-zero length in the first
    const int32_t* kind = HI(BI_con_cvx);
    const float* cax = wf + dir[2 * BF_con_axis];
    int ncyl = 0;
    for (int c = 0; c < v.ncon; ++c) {
      if (kind[c] > -2) continue;
      if (c >= v.ncon - v.npair) return bad("a cylinder slot among the pair contacts");
      if (kind[c] == -2) {
        if (c + 2 >= v.ncon - v.npair || kind[c + 1] != -3 || kind[c + 2] != -4) return bad("a cylinder needs three consecutive ground-contact slots");
        if (!(cax[3 * c] * cax[3 * c] + cax[3 * c + 1] * cax[3 * c + 1] + cax[3 * c + 2] * cax[3 * c + 2] > 0.f)) return bad("a cylinder with a zero half-axis");
        ++ncyl;
      } else if (c == 0 || kind[c - 1] != kind[c] + 1) return bad("a cylinder's second / third slot without its first");
    }
    if (ncyl != wi[36]) return bad("header ncyl does not match the contact table");
    v.ncyl = ncyl;
  }
  {
    // the hull section: every index the kernel follows from a pair row to a hull, its faces, their vertex lists and its edges
    v.hull_words = (int)hull_words;
    const int32_t* hs = wi + total;
    HullView hv{};
    if (hull_words > 0) {
      if (hull_words < 8 || (hull_words & 3)) return bad("hull section too short");
      if (hs[0] < 1 || hs[1] < 4 || hs[2] < 4 || hs[3] < 12 || hs[4] < 6 || hs[0] > 64 || hs[1] > 64 * 64 || hs[2] > 128 * 64 || hs[3] > 6 * 128 * 64 || hs[4] > 192 * 64)
        return bad("hull section: dimension out of range");
      if (hs[5] < 3 * hs[0] || hs[5] > hs[4]) return bad("hull section: number of edge directions out of range");
      hv = hull_view(hs[0], hs[1], hs[2], hs[3], hs[4], hs[5]);
      if ((size_t)hv.words != hull_words) return bad("hull section: length does not follow from its dimensions");
      {
        const int32_t* ua = hs + hv.udadr;
        if (ua[0] != 0 || ua[hv.nhull] != hv.nudir) return bad("hull section: edge-direction ranges do not cover their array");
        for (int h = 0; h < hv.nhull; ++h) if (ua[h + 1] < ua[h] + 3) return bad("a hull needs at least three edge directions");
      }
      const int32_t *va = hs + hv.vadr, *fa = hs + hv.fadr, *ea = hs + hv.eadr, *pa = hs + hv.face_adr, *fi = hs + hv.fidx, *ed = hs + hv.edge;
      if (va[0] != 0 || fa[0] != 0 || ea[0] != 0 || pa[0] != 0 || va[hv.nhull] != hv.nvert || fa[hv.nhull] != hv.nface || ea[hv.nhull] != hv.nedge || pa[hv.nface] != hv.nfidx)
        return bad("hull section: address tables do not cover their arrays");
      for (int h = 0; h < hv.nhull; ++h) {
        if (va[h + 1] < va[h] + 4 || va[h + 1] - va[h] > 64 || fa[h + 1] < fa[h] + 4 || ea[h + 1] < ea[h] + 6) return bad("a hull needs 4 .. 64 vertices, at least 4 faces and 6 edges");
        for (int f = fa[h]; f < fa[h + 1]; ++f) {
          if (pa[f + 1] < pa[f] + 3 || pa[f + 1] - pa[f] > 64) return bad("a hull face needs 3 .. 64 vertices");
          for (int i = pa[f]; i < pa[f + 1]; ++i) if (fi[i] < va[h] || fi[i] >= va[h + 1]) return bad("hull face vertex out of its hull's range");
        }
        for (int e = 2 * ea[h]; e < 2 * ea[h + 1]; ++e) if (ed[e] < va[h] || ed[e] >= va[h + 1]) return bad("hull edge vertex out of its hull's range");
      }
    }
    const float* pg = wf + dir[2 * BF_pair_geom];
    auto v_pair_body = [&](int k) { const int32_t* pb = HI(BI_pair_body); return ((long long)pb[2 * k] << 32) | (long long)(unsigned)pb[2 * k + 1]; };
    for (int k = 0; k < v.npair; ++k) {
      const float* row = pg + 16 * k;
      const float hid = row[7], slot = row[15];
      // a hull pair (box / mesh against box / mesh, four slots): geom 1 carries no shape of its own and geom 2's radius word names geom 1's hull
      const bool hullpair = hid != 0.f && row[14] != 0.f && row[3] == 0.f && row[4] == 0.f && row[5] == 0.f && row[6] == 0.f;
      if (hid != (float)(int)hid || hid < 0.f || hid > (float)hv.nhull || slot != (float)(int)slot || slot < 0.f || slot > (hullpair ? 3.f : 1.f))
        return bad("pair row: hull / slot tag out of range");
      if (hullpair) {
        const float h1 = row[14];
        if (h1 != (float)(int)h1 || h1 < 1.f || h1 > (float)hv.nhull || h1 == hid) return bad("pair row: a hull pair's first hull out of range");
        if (slot == 0.f && k + 3 >= v.npair) return bad("pair row: a hull pair needs four consecutive slots");
        // (the manifold's candidates are kept four to a lane: faces of at most 16 vertices on either side)
        const int32_t *fa = wi + total + hv.fadr, *pa = wi + total + hv.face_adr;
        for (int hh : {(int)h1 - 1, (int)hid - 1})
          for (int f = fa[hh]; f < fa[hh + 1]; ++f) if (pa[f + 1] - pa[f] > 16) return bad("a hull in a hull pair has a face of more than 16 vertices");
      }
      if (slot >= 1.f && (hid == 0.f || k == 0 || pg[16 * (k - 1) + 7] != hid || pg[16 * (k - 1) + 15] != slot - 1.f || pg[16 * (k - 1) + 14] != row[14] ||
                          v_pair_body(k) != v_pair_body(k - 1)))
        return bad("pair row: a later slot must follow its pair's previous one");
    }
  }
  {
    const int32_t *jt = HI(BI_jnt_type), *qa = HI(BI_jnt_qposadr), *da = HI(BI_jnt_dofadr), *jn = HI(BI_body_jntnum), *ja = HI(BI_body_jntadr),
                  *par = HI(BI_body_parent), *dp = HI(BI_dof_parentid), *la = HI(BI_level_adr);
    const int32_t *dj = HI(BI_dof_jntid), *jb = HI(BI_jnt_bodyid), *jl = HI(BI_jnt_limited), *lj = HI(BI_lim_jntid);
    const float* jr = wf + dir[2 * BF_jnt_range];
    v.nball = 0;
    for (int j = 0; j < v.njnt; ++j) {
      if (jt[j] != JNT_FREE && jt[j] != JNT_BALL && jt[j] != JNT_HINGE && jt[j] != JNT_SLIDE) return bad("unsupported joint type");
      if (jt[j] == JNT_FREE && (qa[j] + 7 > v.nq || da[j] + 6 > v.nv)) return bad("free joint address out of range");
      if (jt[j] == JNT_BALL) {
        // a quaternion and three dofs of its own, alone in its body (its axes are the body's), a limit on the rotation angle: range = (0, max)
        if (qa[j] + 4 > v.nq || da[j] + 3 > v.nv) return bad("ball joint address out of range");
        for (int k = 0; k < 3; ++k) if (dj[da[j] + k] != j) return bad("ball joint: its three dofs must name it in dof_jntid");
        if (jn[jb[j]] != 1 || ja[jb[j]] != j) return bad("a ball joint must be the only joint of its body");
        bool limited = jl[j] != 0;
        for (int r = 0; r < v.nlimit; ++r) limited = limited || lj[r] == j;
        if (limited && !(jr[2 * j] == 0.f && jr[2 * j + 1] > 0.f)) return bad("a limited ball joint needs range = (0, max) with max > 0");
        ++v.nball;
      }
    }
    // (... and nobody else's: the kernel takes a ball dof's place among the three from its distance to the joint's first dof)
    for (int d = 0; d < v.nv; ++d) if (jt[dj[d]] == JNT_BALL && (d < da[dj[d]] || d >= da[dj[d]] + 3)) return bad("ball joint: a dof outside its three names it in dof_jntid");
    for (int b = 1; b < v.nbody; ++b) {
      if (par[b] >= b) return bad("bodies are not topologically ordered");
      if (jn[b] > 0 && (ja[b] < 0 || ja[b] + jn[b] > v.njnt)) return bad("body joint range out of bounds");
    }
    for (int d = 0; d < v.nv; ++d) if (dp[d] >= d) return bad("dof_parentid must point to an earlier dof");
    for (int l = 0; l < v.nlevel; ++l) if (la[l + 1] < la[l] || la[l + 1] > v.nbody - 1) return bad("level_adr not monotone");
    if (HI(BI_root_body)[0] != 1) return bad("body 1 must be the first tree root");
  }
  if (v.cparam) {
    // the contact-parameter section: condim 1 or 3, finite values, solimp inside MuJoCo's clamps (dmin / dmax / mid in [mjMINIMP, mjMAXIMP], width > 0,
    // power >= 1), a positive time constant / damping ratio in standard form, margins finite
    const float* cf = wf + total + hull_words;
    const int32_t* ci = wi + total + hull_words;
    auto fin = [](float x) { return x == x && x - x == 0.f; };
    auto good_ref = [&](const float* r) { return fin(r[0]) && fin(r[1]) && (r[0] <= 0.f || r[1] > 0.f) && (r[0] > 0.f || r[1] <= 0.f); };
    auto good_imp = [&](const float* i) {
      for (int k = 0; k < 5; ++k) if (!fin(i[k])) return false;
      return i[0] >= MJ_MINIMP && i[0] <= MJ_MAXIMP && i[1] >= MJ_MINIMP && i[1] <= MJ_MAXIMP && i[2] > 0.f && i[3] >= MJ_MINIMP && i[3] <= MJ_MAXIMP && i[4] >= 1.f;
    };
    for (int c = 0; c < v.ncon; ++c) {
      if (ci[cpv.con_condim + c] != 1 && ci[cpv.con_condim + c] != 3) return bad("contact-parameter section: condim must be 1 or 3");
      if (!good_ref(cf + cpv.con_solref + 2 * c) || !good_imp(cf + cpv.con_solimp + 5 * c) || !fin(cf[cpv.con_margin + c]))
        return bad("contact-parameter section: a contact slot's solref / solimp / margin is not finite or outside MuJoCo's ranges");
    }
    for (int r = 0; r < v.nlimit; ++r)
      if (!good_ref(cf + cpv.lim_solref + 2 * r) || !good_imp(cf + cpv.lim_solimp + 5 * r) || !fin(cf[cpv.lim_margin + r]))
        return bad("contact-parameter section: a joint limit's solref / solimp / margin is not finite or outside MuJoCo's ranges");
    for (int k = 0; k < v.ncvx; ++k) if (!fin(cf[cpv.cvx_margin + k])) return bad("contact-parameter section: a convex geom's margin is not finite");
  }
  v.blob_words = (int)((total + 3) & ~(size_t)3);
  if ((size_t)v.blob_words != total) return bad("blob length must be a multiple of 4 words");
  for (int k = 0; k < BLOB_ARRAY_COUNT; ++k) v.o[k] = dir[2 * k];
  v.obs_dim = v.nq + 2 * v.nv + (v.include_c ? 16 * (v.nbody - 1) : 0);  // env.py:246-259
  v.obs_pad = (v.obs_dim + 3) & ~3;
  v.rec_dim = v.obs_pad + ((v.nv + 2 + 3) & ~3);
  if (v.neq > 0) {
    // the equality section: every element's kind, bodies / joints and rows, and finite parameters in MuJoCo's ranges - the kernel follows
    // these ids into the tables without another check
    const int32_t* es = wi + eq_at;
    const float* ef = wf + eq_at;
    const EqView ev = eq_view(v.neq, eq_nel);
    auto fin = [](float x) { return x == x && x - x == 0.f; };
    const int32_t* jtype = HI(BI_jnt_type);
    int next_row = 0;
    for (int e = 0; e < eq_nel; ++e) {
      const int32_t* ri = es + ev.rec + kEqRecordWords * e;
      const float* rf = ef + ev.rec + kEqRecordWords * e;
      const int dim = ri[0] == EQ_CONNECT ? 3 : ri[0] == EQ_JOINT ? 1 : 0;
      if (dim == 0) return bad("equality section: an element that is neither connect nor joint");
      if (ri[3] != next_row || ri[3] + dim > v.neq) return bad("equality section: an element's rows are not the next ones");
      for (int k = 0; k < dim; ++k) if (es[ev.row + ri[3] + k] != e) return bad("equality section: a row that is not its element's");
      next_row += dim;
      if (ri[0] == EQ_CONNECT) {
        if (ri[1] < 1 || ri[1] >= v.nbody || ri[2] < 0 || ri[2] >= v.nbody || ri[1] == ri[2]) return bad("equality section: a connect's bodies out of range");
      } else {
        if (ri[1] < 0 || ri[1] >= v.njnt || ri[2] < -1 || ri[2] >= v.njnt || ri[1] == ri[2]) return bad("equality section: a joint equality's joints out of range");
        if (jtype[ri[1]] == JNT_FREE || (ri[2] >= 0 && jtype[ri[2]] == JNT_FREE)) return bad("equality section: a joint equality on a free joint");
        if (jtype[ri[1]] == JNT_BALL || (ri[2] >= 0 && jtype[ri[2]] == JNT_BALL)) return bad("equality section: a joint equality on a ball joint");
      }
      for (int k = 4; k < 23; ++k) if (!fin(rf[k])) return bad("equality section: a value is not finite");
      const float* sr = rf + 15;
      const float* si = rf + 17;
      if ((sr[0] <= 0.f) != (sr[1] <= 0.f) || !(si[0] >= MJ_MINIMP && si[0] <= MJ_MAXIMP && si[1] >= MJ_MINIMP && si[1] <= MJ_MAXIMP && si[2] > 0.f &&
                                                si[3] >= MJ_MINIMP && si[3] <= MJ_MAXIMP && si[4] >= 1.f))
        return bad("equality section: solref / solimp outside MuJoCo's ranges");
      if (!(rf[22] > 0.f)) return bad("equality section: invweight must be positive");
    }
    if (next_row != v.neq) return bad("equality section: the elements' rows do not add up to header word 38");
  }
  *dims = blob_dims_of(v);
  *canon_words = canon.words;
  return MPPO_OK;
}

}  // namespace mppo
