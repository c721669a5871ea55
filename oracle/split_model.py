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
