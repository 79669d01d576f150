"""The MFMA products bit for bit against float64 (k_gemm.hip, k_gemm_lds.hip, the rollout forward, the minibatch gradient).

Every operand is drawn from a small dyadic grid (k/2, k/8, small |k|).  Every product and every partial sum is then exactly
representable in float32 - and in bf16 where a kernel rounds an operand - so the result does not depend on summation order,
tile shape, split-K or MFMA layout: the float64 reference has to be reproduced with NO tolerance.  An element dropped,
duplicated, taken from padding or rounded differently shows up as a difference of at least one grid quantum.

Rules every case follows:
  reference   plain NumPy float64, or oracle/ppo_oracle.py in float64
  guard       asserted from the reference alone, before the kernel's output is looked at: the expected values are float32
              numbers; in bf16 cases every operand a kernel rounds (hidden activations, dZ, weights) has its low 16 float32
              bits zero.  An assert - never a skip or a filter: the grids are chosen so that the reference passes it
  canaries    NaN wherever a kernel must not read or write: between K and lda, between N and ldb / ldc, rows past M, the
              slab tail past (M+1).N, the workspaces.  Outputs are compared as whole buffers, canaries included

Backends: CPU emulator build of the kernel sources (default) and MI355X (-m gpu), like tests/test_kernels_ppo.py.  The
device buffers of a case stay referenced until its result has been read (the calls are asynchronous).
"""

import ctypes as C

import numpy as np
import pytest

from minppo_amd import _native as nat
from oracle import ppo_oracle as po

f32 = np.float32
KS = [32 * f + t for f in range(6) for t in (0, 1, 7, 8, 9, 31) if 32 * f + t > 0]  # 0..5 full k-sets of 32 x every tail of the tail-MFMA count and load_tail
MN = [1, 31, 32, 33, 63, 64, 65, 129]                                               # around the 32-wide wave tile and the 64-wide workgroup tile
# leading dimension / alignment settings (ld from the extent, float offset of the base pointer): they select between the float4 and the dword
# loaders of the direct kernels and between the `fast` and `slow` kernels of the LDS-staged one
LDMODES = 4


def _ld(extent, mode):
    return extent if mode == 0 else (extent + 3) // 4 * 4 + (0 if mode == 1 else 4)


def _off(mode):
    return 1 if mode == 3 else 0  # 4 bytes off a 16-byte boundary


def _grid(rng, shape, q, kmax, density=1.0):
    """k.q with |k| <= kmax, a fraction `density` of them non-zero candidates."""
    k = rng.integers(-kmax, kmax + 1, shape)
    if density < 1.0:
        k = k * (rng.random(shape) < density)
    return (k * q).astype(np.float64)


def _is_f32(x):
    x = np.asarray(x, np.float64)
    return bool(np.isfinite(x).all() and (x.astype(f32).astype(np.float64) == x).all())


def _is_bf16(x):
    x = np.asarray(x, np.float64)
    return _is_f32(x) and bool((np.ascontiguousarray(x, f32).view(np.uint32) & 0xFFFF == 0).all())


def _guard_sums(absbound, q):
    """Every partial sum of a product whose terms are multiples of q is a multiple of q bounded by the sum of the terms' magnitudes:
    exact in float32, in any order, when that bound stays below 2^24 quanta."""
    assert float(np.max(absbound)) / q <= 2 ** 24


class _Mat:
    """A [rows, cols] matrix at leading dimension ld inside a NaN-filled device buffer (one more row and a few floats behind
    it, `off` floats in front of it)."""

    def __init__(self, be, rows, cols, ld, off=0, vals=None):
        self.be, self.rows, self.cols, self.ld, self.off = be, rows, cols, ld, off
        self.img = np.full(off + (rows + 1) * ld + 4, np.nan, f32)
        if vals is not None:
            self.view(self.img)[:rows, :cols] = vals
        self.dev = be.arr(self.img)
        self.ptr = be.ptr(self.dev) + 4 * off

    def view(self, flat):
        return flat[self.off:self.off + (self.rows + 1) * self.ld].reshape(self.rows + 1, self.ld)

    def check(self, want, msg):
        """The whole buffer: `want` in [rows, cols], NaN everywhere else."""
        exp = np.full_like(self.img, np.nan)
        self.view(exp)[:self.rows, :self.cols] = want
        np.testing.assert_array_equal(self.be.host(self.dev), exp, err_msg=msg)


class _Gemm:
    """One problem of an mppo_gemm_batch launch: dyadic operands in NaN-padded buffers, the float64 reference, the guard."""

    def __init__(self, be, rng, variant, M, N, K, mode=0, bf16=0, act=0, bias=False, gather=None, ksplit=1, slab_stride=None, bias_out=True, A=None, B=None,
                 biasv=None, q=0.25):
        self.be, self.variant, self.ksplit = be, variant, ksplit
        self.msg = f"variant {variant} M={M} N={N} K={K} ld mode {mode} bf16={bf16} act={act} bias={bias} gather={gather} ksplit={ksplit}"
        off = _off(mode)
        A = _grid(rng, (M, K), 0.5, 2) if A is None else A          # op(A) [M, K]
        B = _grid(rng, (K, N), 0.5, 2) if B is None else B          # op(B) [K, N]
        assert _is_bf16(A) and _is_bf16(B)                            # (bf16 cases: the kernel's operand rounding changes nothing)
        _guard_sums(np.abs(A) @ np.abs(B) + 1.0, q)                  # terms: multiples of q (k/2 operands: 1/4); + 1 for the bias
        # ---- A: [M, K] rows (variants 0, 1) or stored [K, M] (variant 2); rows optionally picked by index out of a larger NaN-filled matrix
        a_rows, a_cols = (K, M) if variant == 2 else (M, K)
        a_img = A.T if variant == 2 else A
        self.g = None
        if gather:
            src_rows = a_rows + 9
            if gather == "perm":
                g = rng.permutation(src_rows)[:a_rows]
            else:  # repeated indices: the rows that share one have to share their values
                g = rng.integers(0, max(1, a_rows // 2), a_rows) * 2 + 1
            src = np.full((src_rows, a_cols), np.nan)
            uniq = {}
            for r, gi in enumerate(g):
                r0 = uniq.setdefault(int(gi), r)
                a_img[r] = a_img[r0]
                src[gi] = a_img[r]
            A = a_img.T if variant == 2 else a_img
            self.g = be.arr(g.astype(np.int32))
            a_rows, a_img = src_rows, src
        self.A = _Mat(be, a_rows, a_cols, _ld(a_cols, mode), off, a_img)
        # ---- B: [K, N] (variants 0, 2) or stored [N, K] (variant 1)
        b_img = B.T if variant == 1 else B
        self.B = _Mat(be, b_img.shape[0], b_img.shape[1], _ld(b_img.shape[1], mode), off, b_img)
        ldc = _ld(N, mode)
        prod = A @ B
        self.bias = self.aux = None
        desc = dict(bias=0, aux=0, bias_out=0, ldaux=0)
        if variant == 0:
            if bias:
                bv = _grid(rng, (N,), 0.5, 2) if biasv is None else biasv
                self.bias = be.arr(bv.astype(f32))
                prod = prod + bv
                desc["bias"] = be.ptr(self.bias)
            self.pre = prod
            self.want = np.maximum(prod, 0) if act == 2 else prod
        elif variant == 1:
            h = _grid(rng, (M, N), 0.125, 8) if act == 1 else _grid(rng, (M, N), 0.5, 2)  # (relu: a third of them exactly 0 or below)
            self.aux = _Mat(be, M, N, _ld(N, (mode + 1) % LDMODES), 0, h)
            desc.update(aux=self.aux.ptr, ldaux=self.aux.ld)
            self.want = prod * ((1 - h * h) if act == 1 else (h > 0))
        if variant != 2:
            assert _is_f32(self.want), self.msg
            self.C = _Mat(be, M, N, ldc, off)
        else:
            # split-K slabs: slab s = C [M, ldc] followed by the column sums [N], then NaN up to the slab stride
            kper = (-(-K // ksplit) + 31) // 32 * 32
            self.stride = slab_stride or (M + 1) * ldc + 7
            assert self.stride >= M * ldc + N
            self.slabs = []
            for s in range(ksplit):
                k0, k1 = min(K, s * kper), min(K, (s + 1) * kper)
                self.slabs.append((A[:, k0:k1] @ B[k0:k1], B[k0:k1].sum(0)))
                assert _is_f32(self.slabs[-1][0]) and _is_f32(self.slabs[-1][1]), self.msg
            assert np.array_equal(sum(s[0] for s in self.slabs), prod) and np.array_equal(sum(s[1] for s in self.slabs), B.sum(0))
            self.M, self.N, self.ldc, self.has_bias_out = M, N, ldc, bias_out
            self.C = _Mat(be, ksplit, self.stride, self.stride, off)
            if bias_out:
                desc["bias_out"] = self.C.ptr + 4 * M * ldc
        self.desc = nat.GemmDesc(self.A.ptr, self.B.ptr, self.C.ptr, desc["bias"], desc["aux"], be.ptr(self.g), desc["bias_out"], M, N, K, self.A.ld, self.B.ld, ldc,
                                 desc["ldaux"], act)

    def check(self):
        if self.variant != 2:
            self.C.check(self.want, self.msg)
            return
        exp = np.full((self.ksplit, self.stride), np.nan)
        for s, (part, colsum) in enumerate(self.slabs):  # (an empty slab: zeros, not what the workspace held)
            exp[s, :self.M * self.ldc].reshape(self.M, self.ldc)[:, :self.N] = part
            if self.has_bias_out:
                exp[s, self.M * self.ldc:self.M * self.ldc + self.N] = colsum
        self.C.check(exp, self.msg)


def _launch(be, probs, variant, ksplit=1, slab_stride=0, bf16=0):
    descs = (nat.GemmDesc * len(probs))(*[p.desc for p in probs])
    be.lib.gemm_batch(descs, len(probs), variant, ksplit, slab_stride, bf16, be.stream)
    for p in probs:
        p.check()


def _sweep(be):
    """(K, M, N, ld mode, i) of a sweep: every K of KS, then every (M, N) pair of MN, the other coordinates cycling with strides that
    are coprime to the lists' lengths so that every value of each list meets several of the others.  The hardware runs every ld mode."""
    i = 0
    dense = be.name == "hip"
    for K in KS:
        for mode in (range(LDMODES) if dense else [i % LDMODES]):
            yield K, MN[(3 * i + 1) % 8], MN[(5 * i + 2) % 8], mode, i
            i += 1
    for M in MN:
        for N in MN:
            if dense or (i % 2 == 0) or M == 129 or N == 129:
                yield KS[(7 * i + 3) % len(KS)], M, N, i % LDMODES, i
            i += 1


@pytest.mark.parametrize("bf16", [0, 1])
def test_gemm_forward_exact(be, bf16):
    """Variant 0, C = act(A.B + bias): gemm_kernel<false, EPI_BIAS_ACT, bf16> at every K edge, tile edge and loader."""
    rng = np.random.default_rng(100 + bf16)
    for K, M, N, mode, i in _sweep(be):
        _launch(be, [_Gemm(be, rng, 0, M, N, K, mode, bf16, act=(0, 2)[(i // 2) % 2], bias=bool((i // 4 + i) % 2), gather=(None, "perm", "rep")[i % 3])], 0, bf16=bf16)


def test_gemm_backward_dact_exact(be):
    """Variant 1, C = (A.B^T) * act'(aux): relu aux with values at and below 0, tanh aux h = k/8 (1 - h^2 and the product stay exact:
    the guard decides); bf16 is refused."""
    rng = np.random.default_rng(110)
    for K, M, N, mode, i in _sweep(be):
        _launch(be, [_Gemm(be, rng, 1, M, N, K, mode, act=(2, 1)[i % 2])], 1)
    p = _Gemm(be, rng, 1, 33, 31, 40, 0, act=2)
    with pytest.raises(nat.NativeError, match="no bf16 variant of the stand-alone backward product"):
        _launch(be, [p], 1, bf16=1)


@pytest.mark.parametrize("bf16", [0, 1])
def test_gemm_weight_gradient_direct_exact(be, bf16):
    """Variant 2 without a gather, C = A^T.B in split-K slabs: gemm_tn_kernel<bf16>.  Here K is the sample count and M, N the
    operands' widths.  Every slab on its own holds the partial product of its k-range, empty slabs (K < 32.ksplit) hold
    zeros, the slabs sum to the reference, bias_out holds the column sums."""
    rng = np.random.default_rng(120 + bf16)
    for K, M, N, mode, i in _sweep(be):
        ksplit = (1, 2, 3, 8)[(i // 3) % 4]
        p = _Gemm(be, rng, 2, M, N, K, mode, bf16, ksplit=ksplit, bias_out=i % 5 != 4)
        _launch(be, [p], 2, ksplit, p.stride, bf16)
    for K in (1, 31, 33, 65):  # fewer samples than slabs x 32: trailing slabs are empty
        p = _Gemm(be, rng, 2, 33, 65, K, 0, bf16, ksplit=8)
        assert sum(1 for s in p.slabs if not s[0].any()) >= 8 - (K + 31) // 32
        _launch(be, [p], 2, 8, p.stride, bf16)


def test_gemm_weight_gradient_gathered_exact(be):
    """Variant 2 with sample rows picked by index: the LDS-staged kernel, its 16-byte `fast` loaders (aligned operands) and its `slow`
    ones, sample counts of whole 32-row tiles only and with a partial last tile (the index prefetch clamps at kend - 1); bf16 is refused."""
    rng = np.random.default_rng(130)
    i = 0
    for K in (32, 64, 96, 160, 1, 33, 70, 95, 100, 191):
        for ksplit in (1, 3):
            for mode in range(LDMODES):
                M, N = MN[(3 * i + 1) % 8], MN[(5 * i + 2) % 8]
                if be.name == "hip" or i % 2 == 0 or mode in (1, 3):
                    p = _Gemm(be, rng, 2, M, N, K, mode, gather=("perm", "rep")[(i // 2) % 2], ksplit=ksplit)
                    _launch(be, [p], 2, ksplit, p.stride)
                i += 1
    p = _Gemm(be, rng, 2, 33, 31, 40, 1, gather="perm")
    with pytest.raises(nat.NativeError, match="no bf16 variant of the gathered weight-gradient product"):
        _launch(be, [p], 2, 1, p.stride, bf16=1)


SIX = [(129, 65, 191), (1, 1, 1), (33, 129, 40), (64, 31, 96), (65, 64, 7), (31, 33, 129)]  # the grid is sized by the largest M and N: the others leave early


@pytest.mark.parametrize("variant,bf16,ksplit,gather", [(0, 0, 1, None), (0, 1, 1, "rep"), (1, 0, 1, None), (2, 0, 2, None), (2, 1, 3, None), (2, 0, 3, "perm")])
def test_gemm_six_problems_in_one_launch(be, variant, bf16, ksplit, gather):
    rng = np.random.default_rng(140 + variant)
    stride = max((M + 1) * _ld(N, i % LDMODES) + 7 for i, (M, N, K) in enumerate(SIX))
    probs = [_Gemm(be, rng, variant, M, N, K, i % LDMODES, bf16, act=2, bias=i % 2 == 0, gather=gather if i != 4 else None, ksplit=ksplit, slab_stride=stride)
             for i, (M, N, K) in enumerate(SIX)]
    _launch(be, probs, variant, ksplit, stride if variant == 2 else 0, bf16)


def test_gemm_launch_limits(be):
    rng = np.random.default_rng(150)
    p = _Gemm(be, rng, 0, 5, 6, 7)
    descs = (nat.GemmDesc * 7)(*[p.desc] * 7)
    with pytest.raises(nat.NativeError, match="1..6 problems"):
        be.lib.gemm_batch(descs, 7, 0, 1, 0, 0, be.stream)
    with pytest.raises(nat.NativeError, match="split-K only with EPI_STORE"):
        be.lib.gemm_batch(descs, 1, 0, 2, 1000, 0, be.stream)
    p.C.check(np.full((5, 6), np.nan), "a refused launch writes nothing")


def _bf16_rne(x):
    """Round to nearest even at 8 significant bits, restated here on exact integers (x = k/2, |k| < 2^15)."""
    k = np.rint(np.asarray(x) * 2).astype(np.int64)
    a = np.abs(k)
    e = np.where(a > 0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) - 7, 0)  # a = m.2^e with m in [128, 256)
    e = np.maximum(e, 0)
    m, r = a >> e, a & ((1 << e) - 1)
    half = (1 << e) >> 1
    up = (r > half) | ((r == half) & (e > 0) & (m & 1 == 1))
    return np.sign(k) * ((m + up) << e) / 2.0


@pytest.mark.parametrize("variant", [0, 2])
def test_gemm_bf16_operands_round_to_nearest_even(be, variant):
    """The bf16 instantiations round both operands to nearest even.  Operands k/2 with up to 11 significant bits: below, at and
    above the half-way point of the 8-bit grid, ties whose truncation is odd (129.5 -> 130, truncated 129) and even (128.5 -> 128)
    among them.  The float64 product of the rounded operands is exact in float32 (guard), so the kernel must equal it bit for bit;
    a truncating conversion differs on every operand above its grid point, by at least one quantum of the result."""
    rng = np.random.default_rng(160 + variant)
    M, N, K = 33, 65, 33
    A = rng.integers(-600, 601, (M, K)) / 2.0
    B = rng.integers(-600, 601, (K, N)) / 2.0
    A[:, 0], A[:, 1], A[:, 2], A[:, 3] = 129.5, 128.5, -129.5, 130.5   # ties
    B[0], B[1], B[2] = 129.5, -130.5, 257.5
    Ar, Br = _bf16_rne(A), _bf16_rne(B)
    np.testing.assert_array_equal(Ar, po.round_bf16(A)); np.testing.assert_array_equal(Br, po.round_bf16(B))  # two statements of the rounding agree
    assert _is_bf16(Ar) and _is_bf16(Br) and Ar[0, 0] == 130 and Ar[0, 1] == 128 and Ar[0, 2] == -130 and Ar[0, 3] == 130
    trunc = lambda x: (np.ascontiguousarray(x, f32).view(np.uint32) & 0xFFFF0000).view(f32).astype(np.float64)
    assert (np.abs(trunc(A)) < np.abs(Ar)).mean() > 0.1 and not np.array_equal(trunc(A) @ trunc(B), Ar @ Br)  # truncation is another product
    p = _Gemm(be, rng, variant, M, N, K, 1, 1, A=Ar, B=Br, ksplit=2 if variant == 2 else 1)
    if variant == 2:  # bias_out is the float32 column sum of B as stored, not of the MFMA's rounded operand
        kper = (-(-K // 2) + 31) // 32 * 32
        p.slabs = [(part, B[s * kper:(s + 1) * kper].sum(0)) for s, (part, _) in enumerate(p.slabs)]
    # the device holds the UNROUNDED operands; the reference was built from the rounded ones
    for mat, full, T in ((p.A, A, variant == 2), (p.B, B, False)):
        mat.view(mat.img)[:mat.rows, :mat.cols] = full.T if T else full
        be.put(mat.dev, mat.img)
    _launch(be, [p], variant, p.ksplit, p.stride if variant == 2 else 0, 1)


def test_gemm_tanh_epilogue_error(be):
    """act = 1: pre-activations on the k/8 grid over [-12, 12], accumulated exactly, so the only error is fast_tanh against the
    float64 tanh.  Bound: the source's own claim (k_gemm.hip: |abs error| < 2e-7) plus half an ulp of 1 for the float32 result."""
    rng = np.random.default_rng(170)
    M, N, K = 33, 70, 40
    vals = np.arange(-88, 89) / 8.0                                   # A: every grid point of [-11, 11] ...
    A = vals[rng.integers(0, vals.size, (M, K))]
    A.reshape(-1)[:vals.size] = vals
    A[M - 1, 0], A[M - 1, 1] = 11.0, -11.0
    B = np.zeros((K, N))                                              # ... selected (and, behind the first K columns, signed) by B: one non-zero per column
    B[:, :K] = np.eye(K)
    B[rng.integers(0, K, N - K), np.arange(K, N)] = rng.choice([-1.0, 1.0], N - K)
    bias = _grid(rng, (N,), 0.125, 8)                                 # ... and shifted by up to 1
    bias[0], bias[1] = 1.0, -1.0
    p = _Gemm(be, rng, 0, M, N, K, 1, act=1, bias=True, A=A, B=B, biasv=bias, q=1.0 / 8)
    assert p.pre.max() == 12.0 and p.pre.min() == -12.0 and np.unique(p.pre).size >= 177 and _is_f32(p.pre)
    descs = (nat.GemmDesc * 1)(p.desc)
    be.lib.gemm_batch(descs, 1, 0, 1, 0, 0, be.stream)
    got = be.host(p.C.dev)
    inside = np.zeros(got.shape, bool)
    p.C.view(inside)[:M, :N] = True
    assert np.isnan(got[~inside]).all() and not np.isnan(got[inside]).any()  # canaries
    err = np.abs(p.C.view(got)[:M, :N].astype(np.float64) - np.tanh(p.pre)).max()
    print(f"fast_tanh max abs error on [-12, 12] ({be.name}): {err:.3e}")
    assert err <= 2e-7 + 2.0 ** -24, err


# ---- the networks: rollout forward and critic gradient ---------------------------------------------------------------------------------------------
FUSED = [(37, 3, 64), (225, 10, 256), (415, 20, 256), (50, 32, 64), (35, 3, 64), (33, 11, 96)]  # benchmark geometry, two head tiles, widest fused head, thin band, odd A
LAYERWISE = [(40, 4, 512), (30, 31, 48), (30, 32, 48), (52, 45, 64), (800, 6, 256)]


def _net(O, A, H, bf16=0, layers=0):
    return nat.Net(O, (O + 3) // 4 * 4, A, H, 0, bf16, layers)  # use_tanh = 0: a ReLU actor


def _dyadic_params(rng, O, A, H, L=2, bf16=False):
    """Weights and biases k/2, |k| <= 2, log_std = 0.  float: a quarter of the weights non-zero.  bf16: a fixed number of non-zero
    weights per column (6, 4, 8 from the first layer up) - with |obs| <= 1 that bounds |h1| by 7 on the 1/4 grid and |h2| by 29 on
    the 1/8 grid, both below 256 quanta: every hidden activation is a bf16 number, whatever the draw."""
    named = {}
    for pref, last in (("a", A), ("c", 1)):
        for i in range(L + 1):
            n_in, n_out = (O if i == 0 else H), (last if i == L else H)
            if bf16:
                nz = min(n_in, (6, 4, 8)[i])
                W = np.zeros((n_in, n_out))
                rows = np.argsort(rng.random((n_in, n_out)), axis=0)[:nz]
                W[rows, np.arange(n_out)] = rng.choice([-1.0, -0.5, 0.5, 1.0], (nz, n_out))
            else:
                W = _grid(rng, (n_in, n_out), 0.5, 2, density=0.25)
            named[f"{pref}_w{i + 1}"], named[f"{pref}_b{i + 1}"] = W, _grid(rng, (n_out,), 0.5, 2)
    named["log_std"] = np.zeros(A)
    flat = po.named_to_flat(named, O, A, H).astype(f32)
    return flat, named


def _forward_exact(be, O, A, H, n, bf16, layers=0, seed=0):
    rng = np.random.default_rng(1000 + seed)
    net = _net(O, A, H, bf16, layers)
    OP, AP = net.OP, (A + 3) // 4 * 4
    flat, n64 = _dyadic_params(rng, O, A, H, layers or 2, bool(bf16))
    assert be.lib.param_count(C.byref(net)) == flat.size
    obs = np.zeros((n, OP), f32)
    obs[:, :O] = _grid(rng, (n, O), 0.5, 2)
    noise = _grid(rng, (n, A), 0.5, 2)
    m64, ls64, v64, (ha, hc) = po.actor_critic_forward(n64, obs[:, :O].astype(np.float64), False, keep=True)
    # guard
    msg = f"O={O} A={A} H={H} n={n} bf16={bf16} layers={layers}"
    assert all(_is_f32(x) for x in (m64, v64, m64 + noise, *ha, *hc)), msg
    hin = [obs[:, :O].astype(np.float64)] + ha[:-1] + [obs[:, :O].astype(np.float64)] + hc[:-1]
    for h, k in zip(hin + [ha[-1], hc[-1]], [f"a_w{i + 1}" for i in range(len(ha))] + [f"c_w{i + 1}" for i in range(len(hc))] + [f"a_w{len(ha) + 1}", f"c_w{len(hc) + 1}"]):
        _guard_sums(np.abs(h) @ np.abs(n64[k]) + 1.0, 1.0 / 64)  # every term a multiple of 1/16 at the least (three layers of k/2 on k/2)
    if bf16:
        assert all(_is_bf16(x) for x in (*ha, *hc, *[v for k, v in n64.items() if "_w" in k])), msg
    d_flat, d_obs = be.arr(flat), be.arr(obs)
    wsb = be.lib.policy_ws_bytes(C.byref(net), n)
    ws = be.full((wsb // 4 + 4,), np.nan)
    outs = []
    for eps in (np.zeros((n, A)), noise, None):  # zero noise: action == mean; k/2 noise: action == mean + noise; NULL noise: the bootstrap form
        d_noise = None if eps is None else be.arr(eps.astype(f32))
        act, logp, value, mean = be.full((n + 1, A), np.nan), be.full((n + 1,), np.nan), be.full((n + 1,), np.nan), be.full((n + 1, AP), np.nan)
        if eps is None:
            be.lib.policy_forward(C.byref(net), be.ptr(d_flat), n, be.ptr(d_obs), OP, 0, 0, 0, be.ptr(value), 0, be.ptr(ws), wsb, be.stream)
            np.testing.assert_array_equal(be.host(value), np.append(v64, np.nan), err_msg=msg)
            continue
        be.lib.policy_forward(C.byref(net), be.ptr(d_flat), n, be.ptr(d_obs), OP, be.ptr(d_noise), be.ptr(act), be.ptr(logp), be.ptr(value), be.ptr(mean),
                              be.ptr(ws), wsb, be.stream)
        got_mean = be.host(mean)
        np.testing.assert_array_equal(got_mean[:n, :A], m64, err_msg=msg)
        np.testing.assert_array_equal(be.host(value), np.append(v64, np.nan), err_msg=msg)
        np.testing.assert_array_equal(be.host(act), np.vstack([m64 + eps, np.full((1, A), np.nan)]), err_msg=msg)
        assert np.isnan(got_mean[n]).all() and np.isnan(be.host(logp)[n])
        np.testing.assert_allclose(be.host(logp)[:n], po.mvn_log_prob(m64 + eps, m64, ls64), atol=5e-5, err_msg=msg)  # (through log 2 pi: its existing bound)
        outs.append((d_noise, act, logp, value, mean))


@pytest.mark.parametrize("O,A,H", FUSED + LAYERWISE)
def test_policy_forward_exact(be, O, A, H):
    _forward_exact(be, O, A, H, 37, 0)


@pytest.mark.parametrize("layers", [1, 3])
def test_policy_forward_exact_other_depths(be, layers):
    _forward_exact(be, 37, 3, 64, 21, 0, layers)


@pytest.mark.parametrize("O,A,H", FUSED)
def test_policy_forward_exact_bf16(be, O, A, H):
    for n in (1, 15, 16, 17, 33) + ((300,) if be.name == "hip" else ()):  # around the 16-row tile; on the hardware one count above a rollout tile
        _forward_exact(be, O, A, H, n, 1, seed=n)


CRITIC = lambda L: [f"c_{t}{i + 1}" for i in range(L + 1) for t in "wb"]


class _GradCase:
    """One minibatch whose critic gradient is exact: old value = the exact value, target = value - k/2, vf_coef 0.5, row weight 1/mb
    with mb a power of two, stats [0, 1].  The actor's loss head goes through exp: its tensors keep the oracle tolerance."""

    def __init__(self, be, O, A, H, mb, bf16=0, layers=0, seed=0):
        self.be, self.mb, self.bf16 = be, mb, bf16
        self.msg = f"O={O} A={A} H={H} mb={mb} bf16={bf16} layers={layers}"
        assert mb & (mb - 1) == 0
        rng = np.random.default_rng(2000 + seed)
        L = layers or 2
        self.net = net = _net(O, A, H, bf16, layers)
        OP = net.OP
        flat, n64 = _dyadic_params(rng, O, A, H, L, bool(bf16))
        B = mb + 13
        bobs = np.zeros((B, OP), f32)
        bobs[:, :O] = _grid(rng, (B, O), 0.5, 2)
        x64 = bobs[:, :O].astype(np.float64)
        m_, ls_, v_, (ha, hc) = po.actor_critic_forward(n64, x64, False, keep=True)
        bact = (m_ + rng.standard_normal((B, A))).astype(f32)  # (actions around the mean: the log-probabilities stay of order A, as in training)
        assert _is_f32(v_), self.msg
        delta = _grid(rng, (B,), 0.5, 2)
        btgt, bval = v_ - delta, v_
        assert _is_f32(btgt), self.msg
        blp = (po.mvn_log_prob(bact.astype(np.float64), m_, ls_) + 0.3 * rng.standard_normal(B)).astype(f32)
        badv = rng.standard_normal(B).astype(f32)
        self.idx_host = idx = rng.permutation(B)[:mb].astype(np.int32)
        args = (x64[idx], bact[idx].astype(np.float64), bval[idx], blp[idx].astype(np.float64), badv[idx].astype(np.float64), btgt[idx], 0.2, 0.5, 0.0, False)
        _, gr = po.loss_and_grad(n64, *args, adv_mean=0.0, adv_std=1.0 - 1e-8)
        self.lo, self.gr_tol = po.loss_and_grad(n64, *args, adv_mean=0.0, adv_std=1.0 - 1e-8, bf16=bool(bf16))
        # guard: the critic's tensors and everything on the way to them are float32 numbers (bf16 numbers where the bf16 kernels round)
        dz = [(delta[idx] * 0.5 / mb)[:, None]]
        for i in range(L, 0, -1):
            dz.append((dz[-1] @ n64[f"c_w{i + 1}"].T) * (hc[i - 1][idx] > 0))
        for k in CRITIC(L):
            assert _is_f32(gr[k]), (self.msg, k)
            np.testing.assert_array_equal(gr[k], self.gr_tol[k], err_msg=k)  # (bf16: the oracle's operand rounding changed nothing)
        np.testing.assert_array_equal(gr[f"c_w{L + 1}"], hc[-1][idx].T @ dz[0])
        assert all(_is_f32(x) for x in (*dz, *[h[idx] for h in hc])), self.msg
        if bf16:
            assert all(_is_bf16(x) for x in (*dz, *[h[idx] for h in hc], *[n64[k] for k in CRITIC(L) if "_w" in k])), self.msg
        self.want = po.named_to_flat(gr, O, A, H)
        self.tol = po.named_to_flat(self.gr_tol, O, A, H)
        self.slices = po.param_slices(O, A, H, L)
        self.P = flat.size
        self.d = {k: be.arr(v) for k, v in dict(flat=flat, obs=bobs, act=bact, val=bval.astype(f32), lp=blp, adv=badv, tgt=btgt.astype(f32), idx=idx).items()}
        self.stats = be.arr(np.array([0.0, 1.0], f32))
        d = self.d
        self.batch = nat.Batch(be.ptr(d["obs"]), OP, be.ptr(d["act"]), A, be.ptr(d["val"]), be.ptr(d["lp"]), be.ptr(d["adv"]), be.ptr(d["tgt"]))
        self.lc = nat.LossCfg(0.2, 0.5, 0.0)
        self.wsb = be.lib.grad_ws_bytes(C.byref(net), mb)
        fused = C.c_int32(-1)
        be.lib.minibatch_path(C.byref(net), C.byref(self.batch), C.byref(fused))
        self.fused = fused.value

    def run(self, how="plain"):
        be, d, mb = self.be, self.d, self.mb
        ws = be.full((self.wsb // 4 + 4,), np.nan)
        grad, loss4 = be.full((self.P + 4,), np.nan), be.zeros((4,))
        head = (C.byref(self.net), be.ptr(d["flat"]), C.byref(self.batch), be.ptr(d["idx"]))
        tail = (be.ptr(self.stats), 1.0 / mb, C.byref(self.lc), be.ptr(grad), be.ptr(loss4), be.ptr(ws), self.wsb)
        if how == "plain":
            be.lib.minibatch_grad(*head, mb, *tail, be.stream)
        else:
            be.lib.shadow_refresh(C.byref(self.net), be.ptr(d["flat"]), mb, be.ptr(ws), self.wsb, be.stream)
            if how == "shadow":
                be.lib.minibatch_grad_shadow(*head, mb, *tail, be.stream)
            else:
                be.lib.gather_rows(C.byref(self.net), C.byref(self.batch), be.ptr(d["idx"]), mb, be.ptr(ws), self.wsb, 0, be.stream)
                be.lib.minibatch_grad_pre(*head, None, mb, *tail, 0, be.stream)
        got = be.host(grad)
        assert np.isnan(got[self.P:]).all() and not np.isnan(got[:self.P]).any(), self.msg
        for k, (o, s) in self.slices.items():
            sz = int(np.prod(s))
            if k.startswith("c_"):
                np.testing.assert_array_equal(got[o:o + sz], self.want[o:o + sz], err_msg=f"{self.msg} {how}: {k}")
            else:
                rel = 5e-3 if self.bf16 else 1e-4
                np.testing.assert_allclose(got[o:o + sz], self.tol[o:o + sz], rtol=0, atol=rel * np.abs(self.tol[o:o + sz]).max() + 1e-7, err_msg=f"{self.msg} {how}: {k}")
        np.testing.assert_allclose(be.host(loss4), self.lo, rtol=2e-3 if self.bf16 else 1e-5, atol=1e-5 if self.bf16 else 1e-6, err_msg=self.msg)


@pytest.mark.parametrize("O,A,H,mb,bf16,layers", [(37, 3, 64, 16, 0, 0), (225, 10, 256, 64, 0, 0), (35, 3, 64, 32, 0, 0),       # fused float; 35 = 32 + 3: the thin row band
                                                   (40, 4, 512, 32, 0, 0), (37, 3, 64, 64, 0, 1), (37, 3, 64, 16, 0, 3),      # layer-wise: H = 512, one and three hidden layers
                                                   (37, 3, 64, 32, 1, 0), (225, 10, 256, 16, 1, 0), (33, 11, 96, 64, 1, 0)])  # fused bf16
def test_critic_gradient_exact(be, O, A, H, mb, bf16, layers):
    case = _GradCase(be, O, A, H, mb, bf16, layers)
    assert case.fused == (1 if H <= 256 and not layers else 0)
    case.run()


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("how", ["shadow", "pre"])
def test_critic_gradient_exact_through_the_engine_entry_points(be, how, bf16):
    """mppo_minibatch_grad_shadow and mppo_minibatch_grad_pre (for bf16 another row pass, fused_bf16.h, with another order of the
    float32 sums): the same bits."""
    case = _GradCase(be, 37, 3, 64, 32, bf16, seed=7)
    assert case.fused == 1
    case.run(how)


def test_critic_gradient_exact_with_32_rows_per_workgroup(be):
    """The 32-row form of the float row pass, where mppo_minibatch_rows_per_workgroup offers it: on the hardware for H = 256 and more
    16-row tiles than two per CU, in the emulator build from 64 rows on."""
    O, A, H, mb = (225, 10, 256, 4096) if be.name == "hip" else (37, 3, 64, 64)
    case = _GradCase(be, O, A, H, mb, 0, seed=9)
    rows = C.c_int32(-1)
    be.lib.minibatch_rows_per_workgroup(C.byref(case.net), mb, 1, C.byref(rows))
    assert rows.value == 32 and case.fused == 1
    case.run("pre")


def test_gemm_stays_inside_exactly_sized_operands(tmp_path):
    """What no comparison of values can see: a lane outside the tile that reads row R instead of row R - 1 feeds an accumulator row that
    is never stored.  The GEMM kernels of the emulator build as a stand-alone program (tests/emu/gemm_bounds_main.cpp + k_gemm.hip +
    k_gemm_lds.hip, nothing else of the library) under the host's AddressSanitizer, every operand, index list and result in a heap block of
    exactly its size: all variants, float and bf16, gathered or not, tight and padded leading dimensions must end without a report."""
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "gemm_bounds"
    csrc, emu = root / "minppo_amd" / "csrc", root / "tests" / "emu"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address", "-fno-sanitize-recover=all", "-x", "c++", "-DMPPO_EMU=1", f"-I{emu}", f"-I{csrc}",
                        f"-I{root / 'include'}", "-Wno-attributes", "-Wno-unused-value", str(csrc / "k_gemm.hip"), str(csrc / "k_gemm_lds.hip"), str(emu / "emu_runtime.cpp"),
                        str(emu / "gemm_bounds_main.cpp"), "-ldl", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr.replace("WARNING: ASan doesn't fully support makecontext/swapcontext", ""), (r.returncode, r.stderr[-3000:])
    assert r.stdout.strip().endswith("launches: ok"), r.stdout[-1000:]
