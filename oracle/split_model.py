"""numpy model of how the ring GEMM kernels form fp32 products on the 16-bit matrix cores (TEST INFRASTRUCTURE, like the
rest of oracle/: imported by tests/ only, never by the product).

Restates swapnet_amd/csrc/conv_gemm.h (the operand cuts) and conv_ring.hip (the kernels that use them):
  * scale_exp / PC_TOP_A / PC_TOP_B      -- the power-of-two operand scale from the operand's amax
  * split8h + conv_precut_kernel (PL 2)  -- x * 2^k = h + l, h = fp16 (A: truncated, B: nearest), l = fp16(x * 2^k - h) nearest
  * conv_fwd_pc_kernel<..., PL = 2>      -- a b ~ h_a h_b + h_a l_b + l_a h_b in fp32, scales removed as two exact factors
  * split8 (three bf16 planes by truncation) and the six-term product of the weight-gradient kernel
A product of two fp16 (bf16) values is exact in fp32, and the MFMA accumulates in fp32, so a float32 matmul of the plane
matrices models the kernel up to summation order.
"""
import numpy as np

PC_TOP_A, PC_TOP_B = 12, 10


def scale_exp(amax, top):
    """k with amax * 2^k in [2^(top-1), 2^top); 0 for a zero / non-finite operand; clamped to +-100 (conv_gemm.h scale_exp)."""
    amax = np.float32(amax)
    if not (amax > 0) or not np.isfinite(amax):
        return 0
    e = int((amax.view(np.uint32) >> np.uint32(23)) & np.uint32(255)) - 127
    return int(max(-100, min(100, top - 1 - e)))


def _trunc_fp16(x):
    """fp32 -> fp16 toward zero (v_cvt_pkrtz_f16_f32), subnormals kept."""
    h = x.astype(np.float16)                                   # nearest
    hf = h.astype(np.float32)
    over = np.abs(hf) > np.abs(x)                              # rounded away from zero: step one ulp back
    h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float16)


def planes_fp16(x, k, truncate_h):
    xs = (x.astype(np.float32) * np.float32(2.0) ** np.float32(k)).astype(np.float32)
    h = _trunc_fp16(xs) if truncate_h else xs.astype(np.float16)
    l = (xs - h.astype(np.float32)).astype(np.float16)          # x' - h is exact in fp32
    return h.astype(np.float32), l.astype(np.float32)


def matmul_two_plane(a, b, ka=None, kb=None):
    """C = A @ B the way conv_fwd_pc_kernel<PL = 2> forms it.  ka / kb override the amax-derived scale exponents."""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    ka = scale_exp(np.abs(a).max(), PC_TOP_A) if ka is None else ka
    kb = scale_exp(np.abs(b).max(), PC_TOP_B) if kb is None else kb
    ah, al = planes_fp16(a, ka, True)
    bh, bl = planes_fp16(b, kb, False)
    acc = (al @ bh + ah @ bl) + ah @ bh                         # smallest terms first, fp32 accumulate
    return (acc * np.float32(2.0) ** np.float32(-ka)) * np.float32(2.0) ** np.float32(-kb)


def planes_bf16(x):
    """Three bf16 planes by truncation (split8): hi, mid, lo with x = hi + mid + lo + O(2^-24 x)."""
    x = np.asarray(x, np.float32)
    def top16(v):
        return (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    hi = top16(x); r = x - hi
    mid = top16(r); s = r - mid
    lo = top16(s)
    return hi, mid, lo


def matmul_three_plane(a, b):
    ah, am, al = planes_bf16(a); bh, bm, bl = planes_bf16(b)
    return ((al @ bh + ah @ bl) + am @ bm) + ((am @ bh + ah @ bm) + ah @ bh)


def matmul_one_plane(a, b, ka=None, kb=None, truncate=False):
    """C = A @ B the way the one-plane configuration forms it (SWN_PC_PLANES=1 / SWN_WGRAD_PLANES=1, bench.py --precision f16:
    conv_gemm.h split8h1 and conv_ring.hip conv_precut_kernel with one plane): each operand ONE fp16 value of x * 2^k, rounded to nearest, one
    MFMA per product, fp32 accumulation.  `truncate` cuts toward zero instead (what the test of the bias must reject).

    Error per output element.  u = 2^-11 is fp16's unit round-off.  A scaled element x' = x 2^k is either normal (|x'| >= 2^-14:
    |fl(x') - x'| <= u |x'|) or subnormal (spacing 2^-24: |fl(x') - x'| <= 2^-25).  With amax 2^k >= 2^(top-1), 2^-k <= amax 2^(1-top),
    so per element  |da| <= u |a| + e_a,  e_a = amax_a 2^-(24 + top_a)   (top_a = PC_TOP_A = 12: amax 2^-36; weights, PC_TOP_B = 10:
    amax 2^-34).  A product a'b' - ab = da b + a db + da db, so summed over k
        |err| <= (2u + u^2) conv(|a|,|b|) + (1 + u) (e_a conv(1,|b|) + e_b conv(|a|,1)) + e_a e_b conv(1,1) + fp32 accumulation,
    the last below K 2^-24 conv(|a|,|b|) <= 2^-10 conv(|a|,|b|) for K <= 2^14.  The tests hold
        |err| <= 2 (2^-10 conv(|a|,|b|) + e_a conv(1,|b|) + e_b conv(|a|,1))
    per element: the factor 2 covers the u^2, (1 + u) and e_a e_b terms and the accumulation."""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    ka = scale_exp(np.abs(a).max(), PC_TOP_A) if ka is None else ka
    kb = scale_exp(np.abs(b).max(), PC_TOP_B) if kb is None else kb

    def cut(x, k):
        xs = (x * np.float32(2.0) ** np.float32(k)).astype(np.float32)
        return (_trunc_fp16(xs) if truncate else xs.astype(np.float16)).astype(np.float32)

    acc = cut(a, ka) @ cut(b, kb)
    return (acc * np.float32(2.0) ** np.float32(-ka)) * np.float32(2.0) ** np.float32(-kb)


def one_plane_bound(a, b, top_a=PC_TOP_A, top_b=PC_TOP_B):
    """The per-element bound of matmul_one_plane (twice the analytic one; see there), float64."""
    A, B = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64))
    ea, eb = A.max() * 2.0 ** -(24 + top_a), B.max() * 2.0 ** -(24 + top_b)
    return 2.0 * (2.0 ** -10 * (A @ B) + ea * (np.ones_like(A) @ B) + eb * (A @ np.ones_like(B)))


# ---- the Winograd transforms whose planes are stored in pair form (swapnet_amd/csrc/wino.hip) -----------------------------------------
# Toom-Cook / Lavin-Gray minimal filtering F(m x m, r x r) with A = m + r - 1 interpolation points: 0, +-1, +-2, inf for the 6-point
# forms F(4,3) and F(3,4) (same points, so the same B^T), and 0, +-1, 1/2, inf for the 5-point strided form F(4,2).  B^T (A x A)
# transforms an A x A input tile, V = B^T d B; the output transform is Y = A^T M A with A^T (m x A), and its adjoint
# dM = A dY A^T transforms an m x m tile of the output gradient.  A transform writes its planes ALREADY cut into fp16 pairs, so the
# scale is fixed before the plane exists, from the bound  |plane| <= gain * amax(tile),  gain = (largest absolute row sum)^2 of the
# matrix applied on both sides: wino.hip input_gain / dy_gain and the literals of tailw_dy_transform / wino_s2_input_transform.
WINO_BT = {
    "F43": np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                     [0, 4, 0, -5, 0, 1]], np.float64),
    "F42": np.array([[0.5, -1, -0.5, 1, 0], [0, -0.5, 0.5, 1, 0], [0, 0.5, -1.5, 1, 0], [0, -1, 0, 1, 0], [0, 0.5, -1, -0.5, 1]], np.float64),
}
WINO_BT["F34"] = WINO_BT["F43"]
WINO_AT = {
    "F43": np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64),
    "F34": np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 1]], np.float64),
    "F42": np.array([[1, 1, 1, 1, 0], [0, 1, -1, 0.5, 0], [0, 1, 1, 0.25, 0], [0, 1, -1, 0.125, 1]], np.float64),
}
WINO_M = {"F43": 4, "F34": 3, "F42": 4}                                  # output tile = the stride between input tiles
WINO_INPUT_GAIN = {"F43": 100.0, "F34": 100.0, "F42": 9.0}               # what wino.hip hands the input transforms
WINO_DY_GAIN = {"F43": 225.0, "F34": 49.0, "F42": 16.0}                  # ... and the transforms of the output gradient


def wino_matrix(form, which):
    """The matrix applied on both sides: B^T ("input") or A ("dy")."""
    return WINO_BT[form] if which == "input" else WINO_AT[form].T


def wino_true_gain(form, which):
    """max |plane| / amax(tile) over all tiles: the squared largest absolute row sum (attained by the outer product of that row's signs)."""
    return float(np.abs(wino_matrix(form, which)).sum(axis=1).max() ** 2)


def wino_periodic_signs(form, which):
    """Signs p[0..m-1] such that the IMAGE pattern sign(row) = p[(row + pad) % m] (same along columns) puts, in every interior tile,
    the sign pattern under which one plane element reaches its maximum -- or as close as the overlap of neighbouring input tiles
    (stride m < A) allows.  Returns (p, the row sum that pattern attains)."""
    M, m = wino_matrix(form, which), WINO_M[form]
    best = (None, -1.0)
    for row in M:
        p = np.ones(m)
        for j in range(m):
            w = row[j::m]                        # the tile entries that see image residue j
            p[j] = 1.0 if w.sum() >= 0 else -1.0         # (entries of both signs in one class: side with the heavier one)
        full = p[np.arange(M.shape[1]) % m]
        got = abs(float(row @ full))
        # (among rows that attain the same sum, the pattern farthest from zero mean: a zero-mean pattern times a constant cancels in a
        # weight gradient, and a test would compare against a reference that is all round-off)
        if got > best[1] + 1e-12 or (abs(got - best[1]) <= 1e-12 and abs(p.sum()) > abs(best[0].sum())):
            best = (p, got)
    return best


def wino_plane(form, which, tile):
    M = wino_matrix(form, which)
    return M @ np.asarray(tile, np.float64) @ M.T


# ---- a float64 model of a pair-form F(4,3) convolution (3 x 3, stride 1, zero padding 1) ------------------------------------------------
# What the pair form keeps of a plane: every element of V = B^T d B (or dM = A dY A^T) is stored as {h | l << 16}, h = fp16(v 2^k)
# to nearest, l = fp16(v 2^k - h) to nearest, with ONE k per tensor from the bound gain x amax(input) (wino.hip pair_scale_exp, pair4).
# The model transforms in float64, rounds the plane to fp32 (the kernel's registers), cuts it that way, forms the three products
# h h + h l + l h exactly, and transforms back in float64: its error is the error of the FORMAT, nothing else.
WINO_G = {"F43": np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                           [0, 0, 1]], np.float64)}
PAIR_TOP = 15                                                            # gain x amax x 2^k lies in [2^14, 2^15)


def pair_scale_exp(amax, gain):
    """k of wino.hip pair_scale_exp: the fp32 product gain x amax scaled into [2^14, 2^15); 0 for a zero operand; clamped to +-100."""
    m = np.float32(np.float32(amax) * np.float32(gain))
    if not (m > 0) or not (m <= np.float32(3.0e38)):
        return 0
    e = int((m.view(np.uint32) >> np.uint32(23)) & np.uint32(255)) - 127
    return int(max(-100, min(100, PAIR_TOP - 1 - e)))


def pair_cut(v, k):
    """(h, l) of pair4, both back in the plane's own units (float64): h + l is what the GEMM sees of v."""
    xs = (np.asarray(v).astype(np.float32) * np.float32(2.0) ** np.float32(k)).astype(np.float32)
    h = xs.astype(np.float16).astype(np.float32)
    l = (xs - h).astype(np.float16).astype(np.float32)                  # xs - h is exact in fp32
    s = 2.0 ** -k
    return h.astype(np.float64) * s, l.astype(np.float64) * s


def pair_abs_err(amax, gain):
    """The absolute part of a pair-cut element's error, |dv| <= 2^-22 |v| + this.  h is nearest (2^-11 relative), the residual
    r = v' - h is at most 2^-11 |v'| and exact; l = fp16(r) is off by 2^-11 |r| <= 2^-22 |v'| where r is normal and by half a
    subnormal step, 2^-25, where it is not.  With gain amax 2^k >= 2^14, 2^-25 2^-k <= gain amax 2^-39."""
    return float(gain) * float(amax) * 2.0 ** -39


def _f43_input_planes(x):
    """x [N, C, H, W] (H, W % 4 == 0) -> V [36, N Th Tw, C], float64."""
    n, c, h, w = x.shape
    xp = np.pad(np.asarray(x, np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
    d = np.lib.stride_tricks.sliding_window_view(xp, (6, 6), axis=(2, 3))[:, :, ::4, ::4]          # [N, C, Th, Tw, 6, 6]
    bt = WINO_BT["F43"]
    v = np.einsum("ij,ncyxjk,lk->ilnyxc", bt, d, bt)
    return np.ascontiguousarray(v).reshape(36, n * (h // 4) * (w // 4), c)


def _f43_dy_planes(dy):
    """dY [N, Co, H, W] -> dM = A dY A^T per 4 x 4 tile, [36, N Th Tw, Co], float64."""
    n, co, h, w = dy.shape
    t = np.asarray(dy, np.float64).reshape(n, co, h // 4, 4, w // 4, 4)
    a = WINO_AT["F43"].T
    m = np.einsum("ia,noyaxb,lb->ilnyxo", a, t, a)
    return np.ascontiguousarray(m).reshape(36, n * (h // 4) * (w // 4), co)


def _f43_out(mat, n, h, w, absolute=False):
    at = np.abs(WINO_AT["F43"]) if absolute else WINO_AT["F43"]
    co = mat.shape[2]
    m = mat.reshape(6, 6, n, h // 4, w // 4, co)
    y = np.einsum("ai,ilnyxo,bl->noyaxb", at, m, at)
    return np.ascontiguousarray(y).reshape(n, co, h, w)


def _f43_weight_planes(w):
    """w [Co, Ci, 3, 3] -> U = G g G^T, [36, Ci, Co], float64."""
    g = WINO_G["F43"]
    u = np.einsum("ij,ocjk,lk->ilco", g, np.asarray(w, np.float64), g)
    return np.ascontiguousarray(u).reshape(36, w.shape[1], w.shape[0])


def _three_products(ah, al, bh, bl):
    return (np.matmul(al, bh) + np.matmul(ah, bl)) + np.matmul(ah, bh)


def _product_bound(absa, ea, absb, eb):
    """|sum_k (a + da)(b + db) - l_a l_b - a b| per element, for |da| <= 2^-22 |a| + ea, |db| <= 2^-22 |b| + eb and the dropped
    l l term (<= 2^-22 |a| |b|): 3 x 2^-22 |a| |b| + ea |b| + eb |a|, the second-order terms left to the factor 2 of the callers."""
    return 3 * 2.0 ** -22 * np.matmul(absa, absb) + ea * np.matmul(np.ones_like(absa), absb) + eb * np.matmul(absa, np.ones_like(absb))


def wino_pair_conv_fwd(x, w, cut=True):
    """Y = conv3x3(x, w), zero padding 1, as the pair-form F(4,3) route forms it: V cut as pair words with k from 100 x amax(x), the
    weight planes U cut as the GEMM's B operand (two fp16 planes, scale_exp(amax U, PC_TOP_B)).  cut=False: the same algorithm in
    exact float64 (equal to the direct convolution: the check of the matrices above).  The input gradient of the layer is this
    function on (dY, the weights transposed and rotated by 180 degrees)."""
    n, c, h, wd = x.shape
    v, u = _f43_input_planes(x), _f43_weight_planes(w)
    if not cut:
        return _f43_out(np.matmul(v, u), n, h, wd)
    vh, vl = pair_cut(v, pair_scale_exp(np.abs(x).max(), WINO_INPUT_GAIN["F43"]))
    uh, ul = planes_fp16(u, scale_exp(np.abs(u).max(), PC_TOP_B), False)
    s = 2.0 ** -scale_exp(np.abs(u).max(), PC_TOP_B)
    return _f43_out(_three_products(vh, vl, uh.astype(np.float64) * s, ul.astype(np.float64) * s), n, h, wd)


def wino_pair_conv_fwd_bound(x, w):
    """Per output element, TWICE the analytic bound of wino_pair_conv_fwd's error (the way one_plane_bound is derived and doubled):
    the plane errors of _product_bound pushed through |A^T| . |A|.  The factor 2 covers the second-order terms and what a kernel
    adds to the format: fp32 transforms and fp32 accumulation."""
    n, c, h, wd = x.shape
    v, u = np.abs(_f43_input_planes(x)), np.abs(_f43_weight_planes(w))
    ev = pair_abs_err(np.abs(x).max(), WINO_INPUT_GAIN["F43"])
    eu = float(u.max()) * 2.0 ** -(24 + PC_TOP_B)
    return 2.0 * _f43_out(_product_bound(v, ev, u, eu), n, h, wd, absolute=True)


def wino_pair_conv_wgrad(x, dy, cut=True):
    """dW [Co, Ci, 3, 3] of the same layer: dU = V^T dM per plane point, both operands pair words (k from 100 x amax(x) and from
    225 x amax(dY)), dW = G^T dU G."""
    v, m = _f43_input_planes(x), _f43_dy_planes(dy)
    vt = np.ascontiguousarray(v.transpose(0, 2, 1))
    if cut:
        vh, vl = pair_cut(vt, pair_scale_exp(np.abs(x).max(), WINO_INPUT_GAIN["F43"]))
        mh, ml = pair_cut(m, pair_scale_exp(np.abs(dy).max(), WINO_DY_GAIN["F43"]))
        du = _three_products(vh, vl, mh, ml)
    else:
        du = np.matmul(vt, m)
    g = WINO_G["F43"]
    return np.einsum("ij,ilco,lk->ocjk", g, du.reshape(6, 6, x.shape[1], dy.shape[1]), g)


def wino_pair_conv_wgrad_bound(x, dy):
    """Twice the analytic bound of wino_pair_conv_wgrad's error per element of dW (see wino_pair_conv_fwd_bound)."""
    v, m = np.abs(_f43_input_planes(x)), np.abs(_f43_dy_planes(dy))
    ev = pair_abs_err(np.abs(x).max(), WINO_INPUT_GAIN["F43"])
    em = pair_abs_err(np.abs(dy).max(), WINO_DY_GAIN["F43"])
    du = _product_bound(np.ascontiguousarray(v.transpose(0, 2, 1)), ev, m, em)
    g = np.abs(WINO_G["F43"])
    return 2.0 * np.einsum("ij,ilco,lk->ocjk", g, du.reshape(6, 6, x.shape[1], dy.shape[1]), g)


def wino_tiles_reached(shape, pos):
    """Boolean [H, W]: the outputs of the 4 x 4 tiles whose 6 x 6 input patch (rows 4 t - 1 .. 4 t + 4) holds pixel pos = (row, col) --
    in the transform domain one element reaches every output of such a tile, not only the 3 x 3 the convolution itself reaches."""
    h, w = shape
    r = np.zeros((h, w), bool)
    ty = [t for t in range(h // 4) if 4 * t - 1 <= pos[0] <= 4 * t + 4]
    tx = [t for t in range(w // 4) if 4 * t - 1 <= pos[1] <= 4 * t + 4]
    for a in ty:
        for b in tx:
            r[4 * a:4 * a + 4, 4 * b:4 * b + 4] = True
    return r
