"""The per-edge message of TensorProductConvLayer.forward in float64, with a first-order error bound per element (test helper, no conftest).

DEFINITION (reference models/score_model.py:108-114, models/layers.py:34-85), everything in numpy float64:
    a    = edge_attr_[e]            the concatenation of the gathered segments                            [F]
    z    = a W1^T + b1,  h = relu(z)                                       fc.0                           [H]
    w    = h W2^T + b2                                                     fc.3                           [weight_numel]
    f    = the l <= 1 features of x[src(e)] and sh[e]: a0 s0 | (a1 . s1)/sqrt 3 | a0 s1 | a1 s0 | (a1 x s1)/sqrt 2
    msg[e, o] = 1/sqrt(U_b) sum_u f[u, c] w[w_off_b + u n_b + n]           per block b, column n, component c
It reads the unpacked fc.0 / fc.3 weights and the block table of the UNFACTORISED packing.ConvSpec (U, n, C, offsets, feature kinds) - never
packed tiles, planes or G.  The torsion spec (DOT features of sh = [0, t]) and the final_conv spec (f_in = 2 ns) are block tables like any other.

BOUND.  `bound[e, o]` is the first-order composition of the per-stage bounds the project documents (include/ddp_hip.h, ddp_conv_task_t;
tests/test_gpu_parity.py::test_stage_a_plane_forms_against_fp64), multiplier exactly 1.  With W2s = W2 / sqrt(U) (the packed weight),
u = 2^-20 and the absolute sums
    Zb[k]  = sum_j |a_j W1[k, j]| + |b1[k]|
    A1[r]  = sum_k |h_k W2s[r, k]| + |b2s[r]|
    Fb[u,c]= the feature with every product replaced by its absolute value (sum |x| |sh|)
the stages are
    fc.0            dz[k] = u Zb[k] + fl_x sum_j |W1[k, j]| + fl_w sum_j |a_j|
    relu            1-Lipschitz: dh = dz
    fc.3            dw[r] = u A1[r] + sum_k dh_k |W2s[r, k]| + fl_x sum_k |W2s[r, k]| + fl_w sum_k |h_k|
    features        4 2^-24 Fb each (their own fp32 arithmetic)
    contraction     u sum_u Fb A1
    => a feature that stays on the per-edge path contributes   Fb (dw + (u + 4 2^-24) A1)
  A factorised conv computes the scalar-input features through G[src][k, n] = sum_u x_u W2s[(u, n), k] (+ Gb from b2s):
    stage A         u sum_u |x_u W2s|  on G
    G as stored     s |G|, s = 0 (fp32 rows), 2^-21 (plane form 0), 2^-19 (plane form 1); absolute fl_g = 2^-30 in the rows kernels, and
                    2^-24 / 32 more in plane form 1 (below |32 G| = 2^-14 the hi word alone)
    h @ G           u sum_k |h_k G_k|,  the error of h: sum_k dh_k |G_k|,  the floor of h: fl_x sum_k |G_k|
    => such a feature contributes   Fb ((2 u + s + 4 2^-24) A1 + sum_k dh_k |W2s| + fl_x sum_k |W2s|)  and, once per element,
       |sh factor| fl_g sum_k |h_k|
  Floors (include/ddp_hip.h:190-195): rows kernels fl_x = 2^-29 (edge_attr_, h), fl_w = 2^-33 (weights), fl_g = 2^-30; the 64- / 32-edge h2 form
  2^-35 per product of a small operand element (K 2^-35 max|w| summed over a row); none in the fp32 forms.  A floor is the error of an element
  whose lo half is a subnormal fp16 number: it is charged only for nonzero elements below the magnitude the header names (|v S| < 2^-3; h2:
  |v| < 2^-14; plane form 1 of G: |32 G| < 2^-14) - zero is exact and larger elements are covered by the relative terms.
`bound` = rel + floor is returned with its two parts, and with the plain sums of absolute terms per element (direct features / G features):
the sharp probe's bound is a multiple of those.

EMULATION (used by tests/test_conv_ref64_cpu.py only; no GPU assertion uses it): the operand roundings the header documents - unified
fp16 hi + lo planes at a scale S, the v = hi + lo / 2048 form, and G in plane form 1 (hi truncated to fp16 + 8 continuation bits).
"""
from collections import namedtuple

import numpy as np

F_SCALAR_S0, F_DOT, F_SCALAR_S1, F_VEC_S0, F_CROSS = range(5)     # feature kinds of packing.BlockSpec.segs (include/ddp_hip.h)
U20 = 2.0 ** -20
FEAT = 4 * 2.0 ** -24
ROWS_SX, ROWS_SW, ROWS_SH, ROWS_SG, GH_SX, GH_SW = 16.0, 256.0, 16.0, 32.0, 2.0, 0.5     # DDP_ROWS_S*, DDP_GH_SX, packing.GH_SW

# kernel: "fp32" (exact fp32 MFMA chains), "h2" (v = hi + lo / 2048 in the 64- / 32-edge kernels), "rows" (unified planes);
# factorized: scalar-input features through G; gh_fmt: plane form of G in the rows kernels
Form = namedtuple("Form", "kernel factorized gh_fmt", defaults=(False, 0))
Ref = namedtuple("Ref", "msg bound rel floor terms_direct terms_g")


def f64(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float64)


def gather_edge_attr(segs):
    """segs: [(rows [*, >= n], idx [E], n)] -> edge_attr_ [E, sum n] float64."""
    return np.concatenate([f64(t)[np.asarray(idx, dtype=np.int64), :n] for t, idx, n in segs], axis=1)


def _features(seg, xs, sh, C):
    """One feature segment (kind, in_off, count) -> (f, fabs) [E, count, C]."""
    kind, off, cnt = seg
    s0, s1 = sh[:, 0], sh[:, 1:4]
    if kind in (F_SCALAR_S0, F_SCALAR_S1):
        a = xs[:, off:off + cnt]
        if kind == F_SCALAR_S0:
            f = (a * s0[:, None])[:, :, None]
        else:
            f = a[:, :, None] * s1[:, None, :]
        return f, np.abs(f)
    a = xs[:, off:off + 3 * cnt].reshape(-1, cnt, 3)
    if kind == F_DOT:
        p = a * s1[:, None, :] / np.sqrt(3.0)
        return p.sum(-1)[:, :, None], np.abs(p).sum(-1)[:, :, None]
    if kind == F_VEC_S0:
        f = a * s0[:, None, None]
        return f, np.abs(f)
    s = np.broadcast_to(s1[:, None, :], a.shape)
    f = np.cross(a, s) / np.sqrt(2.0)
    i, j = [1, 2, 0], [2, 0, 1]
    fabs = (np.abs(a[..., i] * s[..., j]) + np.abs(a[..., j] * s[..., i])) / np.sqrt(2.0)
    assert C == 3
    return f, fabs


def _mm(hh, Ws):
    """[E, H] x [U, n, H] -> [E, U, n]."""
    U, n, H = Ws.shape
    return (hh @ Ws.reshape(U * n, H).T).reshape(-1, U, n)


def _contract(f, w):
    """f [E, U, C], w [E, U, n] -> [E, n, C]."""
    return np.matmul(f.transpose(0, 2, 1), w).transpose(0, 2, 1)


def hidden(ea, W1, b1):
    """(z, Zb) of fc.0."""
    return ea @ W1.T + b1, np.abs(ea) @ np.abs(W1).T + np.abs(b1)


def reference(spec, W1, b1, W2, b2, ea, xs, sh, form=Form("fp32")):
    """spec: the unfactorised packing.ConvSpec; W1 [H, F], b1 [H], W2 [weight_numel, H], b2: the fc weights; ea [E, F] = edge_attr_,
    xs [E, D_in] = x[src], sh [E, 4] per edge.  -> Ref(msg, bound, rel, floor, terms_direct, terms_g), all [E, d_out] float64."""
    W1, b1, W2, b2, ea, xs, sh = (f64(t) for t in (W1, b1, W2, b2, ea, xs, sh))
    E = ea.shape[0]
    rows, h2 = form.kernel == "rows", form.kernel == "h2"
    # an operand element carries its absolute floor only where it is nonzero and below the magnitude at which its lo half stays a normal
    # fp16 number: |v S| < 2^-3 for the unified planes (floor 2^-25 / S), |v| < 2^-14 for v = hi + lo / 2048 (floor 2^-35, both operands)
    fl_x, fl_w, th_x, th_w = (2.0 ** -25 / ROWS_SX, 2.0 ** -25 / ROWS_SW, 2.0 ** -3 / ROWS_SX, 2.0 ** -3 / ROWS_SW) if rows else \
        (2.0 ** -35, 2.0 ** -35, 2.0 ** -14, 2.0 ** -14) if h2 else (0.0, 0.0, 0.0, 0.0)
    s_g = (2.0 ** -19 if form.gh_fmt == 1 else 2.0 ** -21) if rows else 0.0
    small = lambda v, th: ((np.abs(v) > 0) & (np.abs(v) < th)).astype(np.float64)      # noqa: E731
    z, Zb = hidden(ea, W1, b1)
    h = np.maximum(z, 0.0)
    habs = np.abs(h)
    dz = fl_x * (small(ea, th_x) @ np.abs(W1).T) + fl_w * (np.abs(ea) @ small(W1, th_w).T)          # the floors' part of dh
    h_small = small(h, th_x)
    out = [np.zeros((E, spec.d_out)) for _ in range(5)]
    msg, rel, floor, td, tg = out
    for b in spec.blocks:
        n, C = b.n, b.C
        u0 = 0
        for seg in b.segs:
            cnt = seg[2]
            f, fabs = _features(seg, xs, sh, C)                                          # [E, cnt, C]
            r = b.w_off + (u0 + np.arange(cnt))[:, None] * n + np.arange(n)[None, :]     # [cnt, n] rows of fc.3
            Ws = W2[r] * b.scale                                                         # [cnt, n, H]
            bs = b2[r] * b.scale
            aWs = np.abs(Ws)
            w = _mm(h, Ws) + bs[None]
            A1 = _mm(habs, aWs) + np.abs(bs)[None]
            Dh_rel = _mm(U20 * Zb, aWs)                                                  # the relative part of dh through |W2s|
            w_fl = _mm(dz + fl_x * h_small, aWs)                                         # the floors of dh and of h itself through |W2s|
            is_g = form.factorized and seg[0] in (F_SCALAR_S0, F_SCALAR_S1)
            if is_g:
                rel_w = (2 * U20 + s_g + FEAT) * A1 + Dh_rel
            else:
                rel_w = (2 * U20 + FEAT) * A1 + Dh_rel
                w_fl = w_fl + fl_w * _mm(habs, small(Ws, th_w))
            sl = slice(b.out_off, b.out_off + n * C)
            put = lambda x: x.reshape(E, n * C)                                          # noqa: E731  ([E, n, C] -> columns 3 n + c)
            msg[:, sl] += put(_contract(f, w))
            rel[:, sl] += put(_contract(fabs, rel_w))
            floor[:, sl] += put(_contract(fabs, w_fl))
            (tg if is_g else td)[:, sl] += put(_contract(fabs, A1))
            if is_g and rows:
                # G as stored: 2^-25 / 32 below |32 G| = 2^-3 (the lo word subnormal); plane form 1: 2^-24 / 32 below |32 G| = 2^-14 (hi alone)
                Gs = (xs[:, seg[1]:seg[1] + cnt] @ Ws.reshape(cnt, n * Ws.shape[2])).reshape(E, n, -1)          # G[src(e)][n, k]
                fg = 2.0 ** -25 / ROWS_SG * small(Gs, 2.0 ** -3 / ROWS_SG)
                if form.gh_fmt == 1:
                    fg = fg + 2.0 ** -24 / ROWS_SG * small(Gs, 2.0 ** -14 / ROWS_SG)
                fl_g = np.einsum("ek,enk->en", habs, fg)
                sfac = np.abs(sh[:, :1]) if seg[0] == F_SCALAR_S0 else np.abs(sh[:, 1:4])       # [E, C]
                floor[:, sl] += put(fl_g[:, :, None] * sfac[:, None, :])
            u0 += cnt
        assert u0 == b.U
    return Ref(msg, rel + floor, rel, floor, td, tg)


def probe_bound(ref, form):
    """The sharp probe's bound (sparse inputs: every element a sum of at most three chains of single multiplications):
    (p 2^-21 + 8 2^-24) sum|terms| with p split operands in the chain - edge_attr_, the fc.0 weight, h, the fc.3 weight: 4; through G stage A's
    two operands replace the fc.3 weight (5) and the storage term is added; 12 2^-24 sum|terms| in the fp32 forms - plus the header's
    absolute floors (ref.floor: zero in the fp32 forms; in the band 2^-3 ... 2^3 every lo half is a normal fp16 number except those of the
    smallest G values, |32 G| < 2^-3, whose floor 2^-30 stays - up to a quarter of the bound on such an element, nothing beside the 2^-11
    of a lost plane)."""
    if form.kernel == "fp32":
        return 12 * 2.0 ** -24 * (ref.terms_direct + ref.terms_g) + ref.floor
    rows = form.kernel == "rows"
    s_g = (2.0 ** -19 if form.gh_fmt == 1 else 2.0 ** -21) if rows else 0.0
    return (4 * 2.0 ** -21 + 8 * 2.0 ** -24) * ref.terms_direct + (5 * 2.0 ** -21 + 8 * 2.0 ** -24 + s_g) * ref.terms_g + ref.floor


# ------------------------------------------------------------------------------------------------ sharp probe inputs
def probe_inputs(spec, d_in, n_channels, channel_cols, lo=-3.0, hi=3.0, seed=0):
    """Sparse inputs of the sharp probe for a conv of block table `spec`: every edge's edge_attr_ has ONE nonzero column j(e), fc.0 is a scaled
    permutation pattern (one k per j, the signs chosen so that h > 0), b1 = b2 = 0, fc.3 dense, every source node's x has ONE nonzero input
    channel (channel_cols[c] = its columns: one for a scalar, three for a vector channel), cycled over all channels.  Magnitudes log-uniform in
    [2^lo, 2^hi], random signs.  E = max(F, H, channels) edges in source order, one node per channel.
    -> dict(W1, b1, W2, b2, ea [E, F], x [N, d_in], src [E], sh [E, 4]) float32 arrays (the values the kernels get)."""
    rng = np.random.default_rng(seed)
    F, H = spec.f_in, spec.hid

    def mag(*shape):
        return np.exp2(rng.uniform(lo, hi, shape)) * rng.choice([-1.0, 1.0], shape)

    E, N = max(F, H, n_channels), n_channels
    perm = rng.permutation(H)[:F] if H >= F else rng.integers(0, H, F)
    sgn = rng.choice([-1.0, 1.0], F)
    W1 = np.zeros((H, F))
    W1[perm, np.arange(F)] = np.abs(mag(F)) * sgn
    j = rng.permutation(E) % F
    ea = np.zeros((E, F))
    ea[np.arange(E), j] = np.abs(mag(E)) * sgn[j]
    W2 = mag(spec.weight_numel, H)
    x = np.zeros((N, d_in))
    for c in range(N):
        cols = channel_cols[c]
        x[c, cols] = mag(len(cols))
    src = np.sort(np.arange(E) % N)
    v = rng.normal(size=(E, 3))
    sh = np.concatenate([np.ones((E, 1)), np.sqrt(3.0) * v / np.linalg.norm(v, axis=1, keepdims=True)], 1)
    f32 = lambda a: a.astype(np.float32)      # noqa: E731
    return dict(W1=f32(W1), b1=np.zeros(H, np.float32), W2=f32(W2), b2=np.zeros(spec.weight_numel, np.float32), ea=f32(ea), x=f32(x),
                src=src.astype(np.int64), sh=f32(sh))


def channel_columns(in_mul):
    """Columns of every input channel of irreps (m0e, m1o, m1e, m0o): scalars one column, vectors three."""
    m0e, m1o, m1e, m0o = in_mul
    cols, o = [], 0
    for m, d in ((m0e, 1), (m1o, 3), (m1e, 3), (m0o, 1)):
        for _ in range(m):
            cols.append(list(range(o, o + d)))
            o += d
    return cols


# ------------------------------------------------------------------------------------------------ operand rounding, emulated
def _h(v):
    return np.asarray(v, dtype=np.float64).astype(np.float16).astype(np.float64)


def split_unified(v, S, lo_scale=1.0, drop_lo=False):
    """v as unified fp16 planes at scale S (V = v S = hi + lo, lo = fp16(V - hi): 22 bits while lo is normal, absolute 2^-25 / S below)
    -> the value the planes stand for.  Mutations: drop_lo (hi only), lo_scale (the lo plane taken at another scale)."""
    V = np.asarray(v, dtype=np.float64) * S
    hi = _h(V)
    lo = _h(V - hi)
    return (hi + (0.0 if drop_lo else lo * lo_scale)) / S


def split_h2(v, drop_lo=False):
    """v = hi + lo / 2048 (w1h / w2h of the 64- and 32-edge kernels)."""
    v = np.asarray(v, dtype=np.float64)
    hi = _h(v)
    lo = _h((v - hi) * 2048.0)
    return hi + (0.0 if drop_lo else lo / 2048.0)


def g_plane_form1(V, ignore_byte=False):
    """V in plane form 1: rounded to 19 significant bits, hi = that truncated to fp16, then 8 continuation bits; below the fp16 normal range
    (|V| < 2^-14) the hi word alone.  ignore_byte: the mutation that decodes hi only."""
    V = np.asarray(V, dtype=np.float64)
    m, e = np.frexp(V)                                  # V = m 2^e, 0.5 <= |m| < 1
    r19 = np.ldexp(np.round(np.ldexp(m, 19)), e - 19)   # 19 significant bits
    m2, e2 = np.frexp(r19)
    hi = np.ldexp(np.trunc(np.ldexp(m2, 11)), e2 - 11)  # truncated to fp16's 11
    sub = np.abs(V) < 2.0 ** -14
    small = np.ldexp(np.round(np.ldexp(V, 24)), -24)    # a subnormal fp16: multiples of 2^-24
    return np.where(sub, small, hi if ignore_byte else r19)


def emulate(spec, W1, b1, W2, b2, ea, xs_of, src, sh, form, mutate=None, swap=None):
    """The definition evaluated on operands rounded as the kernel form documents (products and sums exact).  xs_of: x [N, D_in]; src [E].
    mutate: None | "drop_lo" | "ignore_byte" | "w2_lo_scale"; swap: (e0, e1) reads x of each other's source node (one wrong row).
    Factorised forms: G is formed per source node from stage A's rounded operands and stored in the plane form."""
    W1, b1, W2, b2, ea, x, sh = (f64(t) for t in (W1, b1, W2, b2, ea, xs_of, sh))
    src = np.asarray(src, dtype=np.int64).copy()
    if swap is not None:
        src[swap[0]], src[swap[1]] = src[swap[1]], src[swap[0]]
    drop = mutate == "drop_lo"
    if form.kernel == "rows":
        rx = lambda v: split_unified(v, ROWS_SX, drop_lo=drop)                          # noqa: E731
        rw = lambda v: split_unified(v, ROWS_SW, drop_lo=drop)                          # noqa: E731
        rw2 = lambda v: split_unified(v, ROWS_SW, drop_lo=drop, lo_scale=1.0 / 2048.0 if mutate == "w2_lo_scale" else 1.0)   # noqa: E731
    elif form.kernel == "h2":
        rx = rw = rw2 = lambda v: split_h2(v, drop_lo=drop)                             # noqa: E731
    else:
        rx = rw = rw2 = lambda v: v                                                     # noqa: E731
    E = ea.shape[0]
    h = rx(np.maximum(rx(ea) @ rw(W1).T + b1, 0.0))
    msg = np.zeros((E, spec.d_out))
    xs = x[src]
    for b in spec.blocks:
        n, C, u0 = b.n, b.C, 0
        for seg in b.segs:
            cnt = seg[2]
            f, _ = _features(seg, xs, sh, C)
            r = b.w_off + (u0 + np.arange(cnt))[:, None] * n + np.arange(n)[None, :]
            Ws, bs = W2[r] * b.scale, b2[r] * b.scale
            sl = slice(b.out_off, b.out_off + n * C)
            if form.factorized and seg[0] in (F_SCALAR_S0, F_SCALAR_S1):
                xa = x[:, seg[1]:seg[1] + cnt]
                if form.kernel == "rows":      # stage A's unified planes of x and W, the product stored in the plane form
                    Gn = np.einsum("ju,unk->jnk", split_unified(xa, GH_SX, drop_lo=drop), split_unified(Ws, ROWS_SG * GH_SW, drop_lo=drop))
                    V = Gn * ROWS_SG
                    Gn = (g_plane_form1(V, ignore_byte=mutate == "ignore_byte") if form.gh_fmt == 1 else split_unified(V, 1.0, drop_lo=drop)) / ROWS_SG
                else:
                    Gn = np.einsum("ju,unk->jnk", xa, Ws)
                t = np.einsum("ek,enk->en", h, Gn[src]) + (xa @ bs)[src]
                sfac = sh[:, :1] if seg[0] == F_SCALAR_S0 else sh[:, 1:4]
                msg[:, sl] += (t[:, :, None] * sfac[:, None, :]).reshape(E, n * C)
            else:
                w = _mm(h, rw2(Ws)) + bs[None]
                msg[:, sl] += _contract(f, w).reshape(E, n * C)
            u0 += cnt
    return msg
