"""
The recurrence kernels (csrc/rnn.hip, gru.hip, lstm_step.hip on csrc/rnn_step.h) restated for their path tests: the host
dispatch as plain functions, float64 one-step references with derived bounds, an fp32 emulation of one step that follows
the pipeline's k order, and the PATHS tables.  tests/test_oracle_rnn_paths.py pins all of it on the CPU,
tests/test_rnn_paths_gpu.py runs every row through the C ABI.  TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

1. DISPATCH.  lstm_resident_ok, pick_rt, resident_lds, stepped_ws, lstm_step_fwd_width, lstm_step_bwd_vec, gru_vec_ok and
   step_grid are the host functions of the three files with pointers replaced by their byte residues (any number congruent
   to the address modulo 16).  chunk_plan(P, K, fwd) is the k loop of a pass: per LDS chunk (kc, klen, kpad), the number of
   prefetch groups of 32 PF k and the 32-k blocks in the last group (mma_chunk breaks out of a partial group at
   `k0 + 32 j >= kpad`).  The GRU's backward runs this plan once per gate block (dz, dr from zg; dhh r from qh).

2. ONE-STEP REFERENCES.  The kernels store every intermediate of the forward walk (gates in zg, cseq, hseq, the GRU's qh), so
   step t is recomputed in float64 from the DEVICE'S OWN state of step t -+ 1: no error accumulates over T and every step of
   every direction is judged on a single-step bound.  lstm_fwd_ref / gru_fwd_ref do this for all t at once (row t of hseq is
   h_{t-1} of the forward direction, row t + 2 is h_{t+1} of the reverse one).  Backward keeps no per-step carry, so
   lstm_bwd_ref / gru_bwd_ref are float64 chains seeded from the device's forward state and the given dh_seq / dh_last; their
   bound is carried along step by step.  They are meant for T <= 4.

3. BOUNDS.  u = 2^-24.  Every value is a pair (v, e): the float64 value and a bound on |device - v|.  An fp32 operation on
   pairs gives e = (first-order propagation, with the second-order cross term for products) (1 + u) + u |v| + 2^-149; the
   operations are applied in the order the source writes them (fp contract is off in all four files).
   Products.  A chain of n roundings over sum a_k b_k has error <= gamma(n) sum |a_k| |b_k| + n 2^-126 (conv2d_np.error_bound;
   gamma(n) = (n + 2) u / (1 - (n + 2) u)), whatever the order of the sum.  How v_mfma_f32_16x16x4_f32 rounds its four terms
   internally is not specified, so EVERY product and EVERY addition is counted as one rounding: n = 2 K for K live k terms
   (K = H forward, 4H backward for the LSTM, 3H for the GRU).  The zero padding up to kpad adds exact zeros and is not
   counted; K comes from chunk_plan (n_fused).  The resident LSTM is a chain of K fmaf starting from the projection:
   n = K + 1.  The stepped LSTM's GEMM sums in an order of its own; n = 2 K covers any order.  Inputs that carry a bound of
   their own (dZ_{t+1} in backward) enter as e |U| plus the sum of absolute values enlarged by e.
   The cell.  sigmoid and tanh have Lipschitz constants 1/4 and 1, so a bound e on the pre-activation becomes e / 4 and e.
   sigm(x) = 1 / (1 + expf(-x)) adds the relative error u (2 EXPF_ULP (1 - s) + 2): expf's error on e^-x weighs e^-x / (1 +
   e^-x) = 1 - s, then the addition and the division round once each.  tanhf adds TANHF_ULP ulp of its result.
   EXPF_ULP = 2 and TANHF_ULP = 4 are TWICE the maximum errors the HIP device math documentation ("HIP math API", single
   precision table) gives for expf (1 ulp) and tanhf (2 ulp) -- the `claim` convention of features_paths_np.ln_pos_bound.
   The table is quoted from memory: the documentation is not part of the build environment.  The constants are not fitted to
   what the kernels return.  Outputs no transcendental touches are judged on the derived bound alone: the GRU's qh and all of
   its backward; the LSTM's backward except for the one tanhf(c_t) of cell_bwd.
   The first step of a direction has no product (h_{-1} = 0): its pre-activation is the projection itself, exactly.  Rows
   with T = 1 therefore isolate the transcendental allowance.

4. EMULATION.  emu_* compute one step in float32 numpy: chunk by chunk, 32-k block by block, MFMA e = 0 .. 7 of a block
   consumes k = k0 + 8 g + e of the four k groups g, here added in the order g = 0, 1, 2, 3, each product and each addition
   rounded.  The resident form is a chain of fused multiply-adds (conv2d_np.fma32), the stepped form a plain k = 0, 1, ..
   sum.  The emulation exists to check the bounds and to plant mutations on the CPU; it is not expected to match the device
   bit for bit.

5. DATA.  draw(): U has entries +-(0.5 .. 1.5) / sqrt(H) ("normal") or +-(1 + 0.1 N(0, 1)) / sqrt(H) ("offset") with random
   signs, so no entry is small and h U stays of order 1 (gates not saturated); projections, biases and incoming gradients are
   N(0, 1) or 1 + 0.1 N(0, 1).
"""
import math

import numpy as np

from oracle.conv2d_np import U as U32, error_bound, fma32, gamma  # noqa: F401

TINY = 2.0 ** -126
DEN = 2.0 ** -149
EXPF_ULP = 2.0                  # 2 x the documented 1 ulp of expf
TANHF_ULP = 4.0                 # 2 x the documented 2 ulp of tanhf
H_TOL = 5e-5                    # the project's absolute bound on h (tests/test_rnn_gpu.py), asserted as well

STEP_ROWS, STEP_UNITS = 64, 16
LSTM_RESIDENT_MAX_H = 80
LSTM_LDS_BUDGET = 160 * 1024


class GruStep:
    NG, PF, KCF, KCB = 3, 1, 256, 768


class LstmStep:
    NG, PF, KCF, KCB = 4, 4, 256, 1024


# ---------------------------------------------------------------------------------------------------- 1. dispatch
def cdiv(a, b):
    return -(-a // b)


def pad16(H):
    return (H + 15) & ~15


def resident_lds(Hp, RT, bwd):
    rw = 4 * RT
    u = Hp * (4 * Hp + 1) * 4
    tile = 2 * rw * 4 * Hp * 4 if bwd else 2 * rw * (Hp + 4) * 4
    return ((u + 15) & ~15) + tile


def lstm_resident_ok(H):
    return int(1 <= H <= LSTM_RESIDENT_MAX_H and resident_lds(pad16(H), 4, True) <= LSTM_LDS_BUDGET)


def pick_rt(B, dirs):
    rt = 1
    while rt < 4:
        if cdiv(B, 4 * rt) * dirs <= 256:
            return rt
        rt *= 2
    return 4


def stepped_ws(B, H, dirs, gemm_rows_workspace):
    """gemm_rows_workspace(M, N, K): the library's lidbox_gemm_rows_workspace (the GEMM family is not restated here)"""
    carry = 2 * dirs * B * H * 4
    g = max(gemm_rows_workspace(B, 4 * H, H), gemm_rows_workspace(B, H, 4 * H))
    return ((carry + 255) & ~255) + g


def lstm_workspace(B, T, H, dirs, gemm_rows_workspace):
    if B <= 0 or T < 1 or H < 1 or dirs < 1 or dirs > 2 or lstm_resident_ok(H):
        return 0
    return stepped_ws(B, H, dirs, gemm_rows_workspace)


def step_workspace(B, T, H, dirs):
    """lidbox_lstm_step_workspace and lidbox_gru_workspace: the carry [dirs][B][H]"""
    if B <= 0 or T < 1 or H < 1 or dirs < 1 or dirs > 2:
        return 0
    return dirs * B * H * 4


def _aligned(nbytes, *residues):
    return all(r % nbytes == 0 for r in residues)


def lstm_step_fwd_width(H, h_rs, U0, U1, hseq):
    if H % 4 == 0 and h_rs % 4 == 0 and _aligned(16, U0, U1, hseq):
        return 4
    if H % 2 == 0 and h_rs % 2 == 0 and _aligned(8, U0, U1, hseq):
        return 2
    return 1


def lstm_step_bwd_vec(U0, U1, zg):
    return _aligned(16, U0, U1, zg)


def gru_vec_ok(H, U0, U1, zg, hseq, qh):
    return H % 4 == 0 and _aligned(16, U0, U1, zg, hseq, qh)


def step_grid(B, H, dirs):
    return (cdiv(B, STEP_ROWS), cdiv(H, STEP_UNITS), dirs)


def chunk_plan(P, K, fwd):
    """the chunks of one k loop of K terms: kc, klen, kpad, prefetch groups, 32-k blocks of the last group"""
    KC = P.KCF if fwd else P.KCB
    out = []
    for kc in range(0, K, KC):
        klen = min(KC, K - kc)
        kpad = (klen + 31) & ~31
        groups = cdiv(kpad, 32 * P.PF)
        out.append(dict(kc=kc, klen=klen, kpad=kpad, groups=groups, last=kpad // 32 - (groups - 1) * P.PF))
    return out


def pass_plan(P, H, fwd):
    """forward: one plan over K = H.  Backward: the LSTM's K = 4H is one contiguous row; the GRU runs K = H per gate block."""
    if fwd:
        return [chunk_plan(P, H, True)]
    if P is LstmStep:
        return [chunk_plan(P, 4 * H, False)]
    return [chunk_plan(P, H, False) for _ in range(3)]


def k_order(plans, H):
    """the live k indices of a pass in the order the MFMAs consume them (gate block q of the GRU's backward at q H)"""
    out = []
    for q, plan in enumerate(plans):
        for c in plan:
            for k0 in range(0, c["kpad"], 32):
                for e in range(8):
                    for g in range(4):
                        k = k0 + 8 * g + e
                        if k < c["klen"]:
                            out.append(q * H + c["kc"] + k)
    return out


def n_fused(P, H, fwd):
    """roundings of one output element's k chain: a product and an addition per live term"""
    return 2 * sum(c["klen"] for plan in pass_plan(P, H, fwd) for c in plan)


def n_of(fam, H, fwd):
    """fam: "step" (lstm_step.hip), "gru", "res" (resident), "stp" (stepped)"""
    if fam == "step":
        return n_fused(LstmStep, H, fwd)
    if fam == "gru":
        return n_fused(GruStep, H, fwd)
    K = H if fwd else 4 * H
    return K + 1 if fam == "res" else 2 * K


def lstm_form(H):
    return "res" if lstm_resident_ok(H) else "stp"


# ---------------------------------------------------------------------------------------------------- 3. bounds
def ulp32(v):
    v = np.abs(np.asarray(v, np.float64))
    return np.where(v >= TINY, 2.0 ** (np.floor(np.log2(np.maximum(v, TINY))) - 23), DEN)


class E:
    """value and bound on the device's distance from it"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    def __getitem__(self, i):
        return E(self.v[i], self.e[i])


def _rnd(v, e):
    return E(v, e * (1.0 + U32) + U32 * np.abs(v) + DEN)


def add(a, b):
    return _rnd(a.v + b.v, a.e + b.e)


def sub(a, b):
    return _rnd(a.v - b.v, a.e + b.e)


def mul(a, b):
    return _rnd(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e)


def one_minus(a):
    return sub(E(np.ones_like(a.v)), a)


def sig(x):
    with np.errstate(over="ignore"):
        v = 1.0 / (1.0 + np.exp(-x.v))
    return E(v, 0.25 * x.e + v * U32 * (2.0 * EXPF_ULP * (1.0 - v) + 2.0) * (1.0 + 1e-6) + TINY)


def tanh_(x):
    v = np.tanh(x.v)
    return E(v, x.e + TANHF_ULP * ulp32(v) + TINY)


def prod(a, Bm, n):
    """a [.., K] (pairs) times the exact matrix Bm [K, N] along a chain of n roundings"""
    Bm = np.asarray(Bm, np.float64)
    Ba = np.abs(Bm)
    return E(a.v @ Bm, a.e @ Ba + error_bound((np.abs(a.v) + a.e) @ Ba, n))


def _where(c, a, b):
    return E(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def _cat(parts, axis=-1):
    return E(np.concatenate([p.v for p in parts], axis), np.concatenate([p.e for p in parts], axis))


def _f64(a):
    return np.asarray(a, np.float64)


def _neighbours(hs, cs, d, T, H):
    """h and c of the step before step t of direction d, for all t: from hseq rows t / t + 2 and cseq shifted by one"""
    lo = 0 if d == 0 else 2
    hp = _f64(hs[:, lo:lo + T, d * H:(d + 1) * H])
    cp = None
    if cs is not None:
        z = np.zeros_like(_f64(cs[d][:, :1]))
        cp = np.concatenate([z, _f64(cs[d][:, :T - 1])], 1) if d == 0 else np.concatenate([_f64(cs[d][:, 1:]), z], 1)
    first = np.zeros((1, T, 1), bool)
    first[0, 0 if d == 0 else T - 1, 0] = True
    return hp, cp, first


# ---------------------------------------------------------------------------------------------------- 2. one-step references
def lstm_fwd_ref(U, zg_in, hs, cs, n):
    """U [dirs] of [H, 4H]; zg_in [dirs, B, T, 4H] the projection; hs [B, T+2, dirs H] and cs [dirs, B, T, H] the STORED state.
    Returns pairs: gates [dirs, B, T, 4H], c and h [dirs, B, T, H]."""
    dirs, B, T, H4 = zg_in.shape
    H = H4 // 4
    G, C, Hh = [], [], []
    for d in range(dirs):
        hp, cp, first = _neighbours(hs, cs, d, T, H)
        x = E(_f64(zg_in[d]))
        pre = _where(first, x, add(x, prod(E(hp), U[d], n)))
        i, f, g, o = sig(pre[..., :H]), sig(pre[..., H:2 * H]), tanh_(pre[..., 2 * H:3 * H]), sig(pre[..., 3 * H:])
        c = add(mul(f, E(cp)), mul(i, g))
        h = mul(o, tanh_(c))
        G.append(_cat([i, f, g, o]))
        C.append(c)
        Hh.append(h)
    st = lambda xs: E(np.stack([x.v for x in xs]), np.stack([x.e for x in xs]))
    return dict(gates=st(G), c=st(C), h=st(Hh))


def gru_fwd_ref(U, brec, zg_in, hs, n):
    """gate order z, r, h; returns pairs gates (z, r, hh) [dirs, B, T, 3H], qh (with its bias) and h [dirs, B, T, H]"""
    dirs, B, T, H3 = zg_in.shape
    H = H3 // 3
    G, Q, Hh = [], [], []
    for d in range(dirs):
        hp, _, first = _neighbours(hs, None, d, T, H)
        b = E(np.broadcast_to(_f64(brec[d]), (B, T, H3)))
        q = _where(first, b, add(prod(E(hp), U[d], n), b))
        x = E(_f64(zg_in[d]))
        z = sig(add(x[..., :H], q[..., :H]))
        r = sig(add(x[..., H:2 * H], q[..., H:2 * H]))
        qh = q[..., 2 * H:]
        hh = tanh_(add(x[..., 2 * H:], mul(r, qh)))
        h = add(mul(z, E(hp)), mul(one_minus(z), hh))
        G.append(_cat([z, r, hh]))
        Q.append(qh)
        Hh.append(h)
    st = lambda xs: E(np.stack([x.v for x in xs]), np.stack([x.e for x in xs]))
    return dict(gates=st(G), qh=st(Q), h=st(Hh))


def _incoming(dh_seq, dh_last, d, t, H, last, shape):
    """the given gradient of h_t as the kernels add it up: dh_seq, then (at the direction's last step) += dh_last"""
    v = E(np.zeros(shape))
    if dh_seq is not None:
        v = E(_f64(dh_seq[:, t, d * H:(d + 1) * H]))
    if dh_last is not None and last:
        l = E(_f64(dh_last[:, d * H:(d + 1) * H]))
        v = add(v, l) if dh_seq is not None else l
    return v


def lstm_cell_bwd_ref(g, ct, cp, dh, dc):
    """cell_bwd of rnn_cell.h on pairs, operation by operation; g = (i, f, g, o) exact, ct, cp exact"""
    ig, fg, gg, og = g
    tc = tanh_(E(ct))
    dct = add(dc, mul(mul(dh, og), one_minus(mul(tc, tc))))
    dz = [mul(mul(mul(dct, gg), ig), one_minus(ig)),
          mul(mul(mul(dct, E(cp)), fg), one_minus(fg)),
          mul(mul(dct, ig), one_minus(mul(gg, gg))),
          mul(mul(mul(dh, tc), og), one_minus(og))]
    return _cat(dz), mul(dct, fg)


def lstm_bwd_ref(U, gates, cs, dh_seq, dh_last, n):
    """float64 chain from the stored forward state: pairs dZ [dirs, B, T, 4H]"""
    dirs, B, T, H4 = gates.shape
    H = H4 // 4
    V, Er = np.zeros(gates.shape), np.zeros(gates.shape)
    for d in range(dirs):
        rec = dc = E(np.zeros((B, H)))
        for s in range(T - 1, -1, -1):
            t = s if d == 0 else T - 1 - s
            tp = t - 1 if d == 0 else t + 1
            dh = _incoming(dh_seq, dh_last, d, t, H, s == T - 1, (B, H))
            if s < T - 1:
                dh = add(rec, dh)
            g = [E(_f64(gates[d, :, t, q * H:(q + 1) * H])) for q in range(4)]
            cp = _f64(cs[d, :, tp]) if s > 0 else np.zeros((B, H))
            dz, dc = lstm_cell_bwd_ref(g, _f64(cs[d, :, t]), cp, dh, dc)
            V[d, :, t], Er[d, :, t] = dz.v, dz.e
            rec = prod(dz, _f64(U[d]).T, n)
    return E(V, Er)


def gru_bwd_ref(U, gates, qh, hs, dh_seq, dh_last, n):
    """pairs dZx = (dz, dr, dhh) [dirs, B, T, 3H] and the h block of dZrec, dhh r, [dirs, B, T, H]"""
    dirs, B, T, H3 = gates.shape
    H = H3 // 3
    V, Er = np.zeros(gates.shape), np.zeros(gates.shape)
    QV, QE = np.zeros(qh.shape), np.zeros(qh.shape)
    for d in range(dirs):
        hpa, _, _ = _neighbours(hs, None, d, T, H)
        rec = carry = None
        for s in range(T - 1, -1, -1):
            t = s if d == 0 else T - 1 - s
            dh = E(np.zeros((B, H))) if rec is None else rec
            if dh_seq is not None:
                x = E(_f64(dh_seq[:, t, d * H:(d + 1) * H]))
                dh = x if rec is None else add(dh, x)
            if dh_last is not None and s == T - 1:
                l = E(_f64(dh_last[:, d * H:(d + 1) * H]))
                dh = l if dh_seq is None else add(dh, l)
            if s < T - 1:
                dh = add(dh, carry)
            z, r, hh = (E(_f64(gates[d, :, t, q * H:(q + 1) * H])) for q in range(3))
            q_ = E(_f64(qh[d, :, t]))
            hp = E(hpa[:, t] if s > 0 else np.zeros((B, H)))
            dz = mul(mul(mul(dh, sub(hp, hh)), z), one_minus(z))
            dhh = mul(mul(dh, one_minus(z)), one_minus(mul(hh, hh)))
            dr = mul(mul(mul(dhh, q_), r), one_minus(r))
            dq = mul(dhh, r)
            carry = mul(dh, z)
            out = _cat([dz, dr, dhh])
            V[d, :, t], Er[d, :, t] = out.v, out.e
            QV[d, :, t], QE[d, :, t] = dq.v, dq.e
            rec = prod(_cat([dz, dr, dq]), _f64(U[d]).T, n)
    return E(V, Er), E(QV, QE)


def chain_fwd(ref, T):
    """the one-step references chained over T: recomputing every step from the stored state T times makes step s exact
    after pass s + 1.  ref(state) -> new state arrays"""
    state = None
    for _ in range(T):
        state = ref(state)
    return state


# ---------------------------------------------------------------------------------------------------- whole layers (CPU pin)
def _sg(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_layer(U, zg_in, dh_seq=None, dh_last=None):
    """float64 Keras LSTM layer from the projection: gates, c, h [dirs, B, T, .] and dZ (w.r.t. the pre-activations)"""
    dirs, B, T, H4 = zg_in.shape
    H = H4 // 4
    G, C, Hs, DZ = (np.zeros((dirs, B, T, w)) for w in (H4, H, H, H4))
    for d in range(dirs):
        Ud = _f64(U[d])
        ts = list(range(T)) if d == 0 else list(range(T - 1, -1, -1))
        h, c = np.zeros((B, H)), np.zeros((B, H))
        for t in ts:
            z = _f64(zg_in[d, :, t]) + h @ Ud
            i, f, g, o = _sg(z[:, :H]), _sg(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), _sg(z[:, 3 * H:])
            c = f * c + i * g
            h = o * np.tanh(c)
            G[d, :, t], C[d, :, t], Hs[d, :, t] = np.concatenate([i, f, g, o], 1), c, h
        if dh_seq is None and dh_last is None:
            continue
        dhn, dcn = np.zeros((B, H)), np.zeros((B, H))
        for j, t in enumerate(reversed(ts)):
            dh = dhn.copy()
            if dh_seq is not None:
                dh += _f64(dh_seq[:, t, d * H:(d + 1) * H])
            if dh_last is not None and j == 0:
                dh += _f64(dh_last[:, d * H:(d + 1) * H])
            i, f, g, o = (G[d, :, t, q * H:(q + 1) * H] for q in range(4))
            tc = np.tanh(C[d, :, t])
            k = ts.index(t)
            cp = C[d, :, ts[k - 1]] if k > 0 else np.zeros((B, H))
            dc = dcn + dh * o * (1 - tc * tc)
            dz = np.concatenate([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
            DZ[d, :, t] = dz
            dcn = dc * f
            dhn = dz @ Ud.T
    return G, C, Hs, DZ


def gru_layer(U, brec, zg_in, dh_seq=None, dh_last=None):
    """float64 Keras GRU layer (reset_after): gates (z, r, hh), qh, h, dZx and the h block of dZrec"""
    dirs, B, T, H3 = zg_in.shape
    H = H3 // 3
    G, Q, Hs, DZ, DQ = (np.zeros((dirs, B, T, w)) for w in (H3, H, H, H3, H))
    for d in range(dirs):
        Ud = _f64(U[d])
        ts = list(range(T)) if d == 0 else list(range(T - 1, -1, -1))
        h = np.zeros((B, H))
        HP = {}
        for t in ts:
            HP[t] = h
            q = h @ Ud + _f64(brec[d])
            x = _f64(zg_in[d, :, t])
            z, r = _sg(x[:, :H] + q[:, :H]), _sg(x[:, H:2 * H] + q[:, H:2 * H])
            hh = np.tanh(x[:, 2 * H:] + r * q[:, 2 * H:])
            h = z * h + (1 - z) * hh
            G[d, :, t], Q[d, :, t], Hs[d, :, t] = np.concatenate([z, r, hh], 1), q[:, 2 * H:], h
        if dh_seq is None and dh_last is None:
            continue
        dhn = np.zeros((B, H))
        for j, t in enumerate(reversed(ts)):
            dh = dhn.copy()
            if dh_seq is not None:
                dh += _f64(dh_seq[:, t, d * H:(d + 1) * H])
            if dh_last is not None and j == 0:
                dh += _f64(dh_last[:, d * H:(d + 1) * H])
            z, r, hh = (G[d, :, t, q * H:(q + 1) * H] for q in range(3))
            dz = dh * (HP[t] - hh) * z * (1 - z)
            dhh = dh * (1 - z) * (1 - hh * hh)
            dr = dhh * Q[d, :, t] * r * (1 - r)
            DZ[d, :, t], DQ[d, :, t] = np.concatenate([dz, dr, dhh], 1), dhh * r
            dhn = dh * z + np.concatenate([dz, dr, dhh * r], 1) @ Ud.T
    return G, Q, Hs, DZ, DQ


def seq_avg_pool_ref(x, alpha):
    """x [B, T, C] float32 -> (out, bound): T - 1 additions, the division, the scale"""
    x = _f64(x)
    T = x.shape[1]
    out = alpha * x.mean(1)
    return out, error_bound(abs(alpha) * np.abs(x).mean(1), T + 1)


def seq_avg_pool_bwd_ref(dout, alpha, T, dx0=None):
    """g = alpha dout / T (two roundings), added to dx0 when accumulating (a third)"""
    g = np.float32(alpha).astype(np.float64) * _f64(dout) / T
    out = np.repeat(g[:, None, :], T, 1)
    bound = 2.5 * U32 * np.abs(out) + DEN
    if dx0 is not None:
        out = out + _f64(dx0)
        bound = bound * (1 + U32) + U32 * np.abs(out)
    return out, bound


# ---------------------------------------------------------------------------------------------------- 4. emulation (fp32)
F = np.float32
MUT_FWD = ("drop_last_k", "drop_first_k2", "unit_shift", "row_shift", "prow_plus_1", "swap_gates")
MUT_BWD = ("drop_last_k", "drop_first_k2", "row_shift", "swap_gates", "omit_dh_last", "omit_carry")


def mut_row(B):
    """the batch row whose A operand the row_shift mutation takes from row b + 1: a tile edge where there is one"""
    for b in (63, 15):
        if b + 1 < B:
            return b
    return B - 2 if B >= 2 else None


def _sig32(x):
    with np.errstate(over="ignore"):
        return (F(1.0) / (F(1.0) + np.exp(-x).astype(F))).astype(F)


def _chain32(A, Bm, order, fam, acc=None, drop=None):
    """acc + A Bm along `order`, in float32: product and addition rounded (MFMA / GEMM), or one fma (resident)"""
    A, Bm = np.ascontiguousarray(A, F), np.ascontiguousarray(Bm, F)
    acc = np.zeros((A.shape[0], Bm.shape[1]), F) if acc is None else acc.astype(F)
    for k in order:
        if k == drop:
            continue
        if fam == "res":
            acc = fma32(A[:, k:k + 1], Bm[k:k + 1, :], acc).astype(F)
        else:
            acc = acc + A[:, k:k + 1] * Bm[k:k + 1, :]
    return acc


def _orders(fam, H, fwd):
    """(k order, chunk plan list) of a pass; the resident and stepped forms walk k = 0, 1, .. as one chunk"""
    if fam in ("step", "gru"):
        plans = pass_plan(LstmStep if fam == "step" else GruStep, H, fwd)
        return k_order(plans, H), plans
    K = H if fwd else 4 * H
    return list(range(K)), [[dict(kc=0, klen=K, kpad=K)]]


def mut_applies(fam, mut, fwd, H, B, T, has_last=False):
    plans = _orders(fam, H, fwd)[1]
    if T < 2 and mut != "omit_dh_last":
        return False                                           # a single step has no product and no carry
    if mut == "drop_first_k2":
        return len(plans[0]) > 1
    if mut == "row_shift":
        return B >= 2
    if mut == "omit_dh_last":
        return has_last
    return True


def _mutate(mut, fam, H, NG, fwd, A, Bm, plans):
    """operands and dropped k of the mutated product.  Bm: U [H, NG H] forward, U^T [NG H, H] backward"""
    drop = None
    if mut == "drop_last_k":
        c = plans[0][0]
        drop = c["kc"] + c["klen"] - 1
    elif mut == "drop_first_k2":
        drop = plans[0][1]["kc"]
    elif mut == "unit_shift":
        Bm = Bm.copy()
        u0 = 16 * ((H - 1) // 16)
        for g in range(NG):
            for u in range(u0, H):
                Bm[:, g * H + u] = Bm[:, (g * H + u + 1) % (NG * H)] if g + 1 < NG or u + 1 < H else 0.0
    elif mut == "row_shift":
        A = A.copy()
        b = mut_row(A.shape[0])
        A[b] = A[b + 1]
    elif mut == "swap_gates":
        Bm = Bm.copy()
        if fwd:
            Bm[:, :H], Bm[:, H:2 * H] = Bm[:, H:2 * H].copy(), Bm[:, :H].copy()
        else:
            Bm[:H], Bm[H:2 * H] = Bm[H:2 * H].copy(), Bm[:H].copy()
    return A, Bm, drop


def emu_lstm_fwd_step(fam, U, zg_in, st, s, mut=None):
    """step s of both directions in float32, from and into st = dict(gates, c, hs) (hs [B, T+2, dirs H], rows 0, T+1 zero)"""
    dirs, B, T, H4 = zg_in.shape
    H = H4 // 4
    order, plans = _orders(fam, H, True)
    for d in range(dirs):
        t = s if d == 0 else T - 1 - s
        prow = t if d == 0 else t + 2
        tp = t - 1 if d == 0 else t + 1
        x = zg_in[d, :, t].astype(F)
        if s > 0:
            A = st["hs"][:, prow + (1 if mut == "prow_plus_1" else 0), d * H:(d + 1) * H]
            A, Bm, drop = _mutate(mut, fam, H, 4, True, A, np.asarray(U[d], F), plans)
            if fam == "res":
                pre = _chain32(A, Bm, order, fam, acc=x, drop=drop)
            else:
                pre = x + _chain32(A, Bm, order, fam, drop=drop)
            cp = st["c"][d, :, tp]
        else:
            pre, cp = x, np.zeros((B, H), F)
        i, f, o = _sig32(pre[:, :H]), _sig32(pre[:, H:2 * H]), _sig32(pre[:, 3 * H:])
        g = np.tanh(pre[:, 2 * H:3 * H]).astype(F)
        c = f * cp + i * g
        st["gates"][d, :, t] = np.concatenate([i, f, g, o], 1)
        st["c"][d, :, t] = c
        st["hs"][:, t + 1, d * H:(d + 1) * H] = o * np.tanh(c).astype(F)


def emu_lstm_fwd(fam, U, zg_in):
    dirs, B, T, H4 = zg_in.shape
    H = H4 // 4
    st = dict(gates=np.zeros(zg_in.shape, F), c=np.zeros((dirs, B, T, H), F), hs=np.zeros((B, T + 2, dirs * H), F))
    for s in range(T):
        emu_lstm_fwd_step(fam, U, zg_in, st, s)
    return st


def emu_gru_fwd_step(U, brec, zg_in, st, s, mut=None):
    """st = dict(gates, qh, hs)"""
    dirs, B, T, H3 = zg_in.shape
    H = H3 // 3
    order, plans = _orders("gru", H, True)
    for d in range(dirs):
        t = s if d == 0 else T - 1 - s
        prow = t if d == 0 else t + 2
        x = zg_in[d, :, t].astype(F)
        b = np.asarray(brec[d], F)[None, :]
        if s > 0:
            hp = st["hs"][:, prow, d * H:(d + 1) * H].copy()
            A = st["hs"][:, prow + 1, d * H:(d + 1) * H] if mut == "prow_plus_1" else hp
            A, Bm, drop = _mutate(mut, "gru", H, 3, True, A, np.asarray(U[d], F), plans)
            q = _chain32(A, Bm, order, "gru", drop=drop) + b
        else:
            hp, q = np.zeros((B, H), F), np.broadcast_to(b, (B, H3)).astype(F)
        z, r = _sig32(x[:, :H] + q[:, :H]), _sig32(x[:, H:2 * H] + q[:, H:2 * H])
        qh = q[:, 2 * H:]
        hh = np.tanh(x[:, 2 * H:] + r * qh).astype(F)
        h = z * hp + (F(1.0) - z) * hh
        st["gates"][d, :, t] = np.concatenate([z, r, hh], 1)
        st["qh"][d, :, t] = qh
        st["hs"][:, t + 1, d * H:(d + 1) * H] = h


def emu_gru_fwd(U, brec, zg_in):
    dirs, B, T, H3 = zg_in.shape
    H = H3 // 3
    st = dict(gates=np.zeros(zg_in.shape, F), qh=np.zeros((dirs, B, T, H), F), hs=np.zeros((B, T + 2, dirs * H), F))
    for s in range(T):
        emu_gru_fwd_step(U, brec, zg_in, st, s)
    return st


def emu_lstm_bwd_step(fam, U, fw, dh_seq, dh_last, bw, s, mut=None):
    """step s of backward in float32.  fw: the forward state (gates, c); bw = dict(dz [dirs, B, T, 4H], dc [dirs, B, H])"""
    dirs, B, T, H4 = fw["gates"].shape
    H = H4 // 4
    order, plans = _orders(fam, H, False)
    one = F(1.0)
    for d in range(dirs):
        t = s if d == 0 else T - 1 - s
        tp = t - 1 if d == 0 else t + 1
        tn = t + 1 if d == 0 else t - 1
        dh = np.zeros((B, H), F)
        if dh_seq is not None:
            dh = dh_seq[:, t, d * H:(d + 1) * H].astype(F)
        if dh_last is not None and s == T - 1 and mut != "omit_dh_last":
            dh = dh + dh_last[:, d * H:(d + 1) * H].astype(F)
        dc = np.zeros((B, H), F)
        if s < T - 1:
            A, Bm, drop = _mutate(mut, fam, H, 4, False, bw["dz"][d, :, tn], np.asarray(U[d], F).T, plans)
            dh = _chain32(A, Bm, order, fam, drop=drop) + dh
            if mut != "omit_carry":
                dc = bw["dc"][d]
        ig, fg, gg, og = (fw["gates"][d, :, t, q * H:(q + 1) * H] for q in range(4))
        ct = fw["c"][d, :, t]
        cp = fw["c"][d, :, tp] if s > 0 else np.zeros((B, H), F)
        tc = np.tanh(ct).astype(F)
        dct = dc + dh * og * (one - tc * tc)
        bw["dz"][d, :, t] = np.concatenate([dct * gg * ig * (one - ig), dct * cp * fg * (one - fg), dct * ig * (one - gg * gg),
                                            dh * tc * og * (one - og)], 1)
        bw["dc"][d] = dct * fg


def emu_lstm_bwd(fam, U, fw, dh_seq, dh_last, upto=0, mut=None):
    """the chain down to step `upto` (inclusive); returns bw"""
    dirs, B, T, H4 = fw["gates"].shape
    bw = dict(dz=np.zeros(fw["gates"].shape, F), dc=np.zeros((dirs, B, H4 // 4), F))
    for s in range(T - 1, upto - 1, -1):
        emu_lstm_bwd_step(fam, U, fw, dh_seq, dh_last, bw, s, mut)
    return bw


def emu_gru_bwd_step(U, fw, dh_seq, dh_last, bw, s, mut=None):
    """fw: forward state (gates, qh, hs); bw = dict(dz [dirs, B, T, 3H], dq [dirs, B, T, H], carry [dirs, B, H])"""
    dirs, B, T, H3 = fw["gates"].shape
    H = H3 // 3
    order, plans = _orders("gru", H, False)
    one = F(1.0)
    for d in range(dirs):
        t = s if d == 0 else T - 1 - s
        prow = t if d == 0 else t + 2
        tn = t + 1 if d == 0 else t - 1
        dh = np.zeros((B, H), F)
        if s < T - 1:
            A = np.concatenate([bw["dz"][d, :, tn, :2 * H], bw["dq"][d, :, tn]], 1)
            A, Bm, drop = _mutate(mut, "gru", H, 3, False, A, np.asarray(U[d], F).T, plans)
            dh = _chain32(A, Bm, order, "gru", drop=drop)
        if dh_seq is not None:
            dh = dh + dh_seq[:, t, d * H:(d + 1) * H].astype(F)
        if dh_last is not None and s == T - 1 and mut != "omit_dh_last":
            dh = dh + dh_last[:, d * H:(d + 1) * H].astype(F)
        if s < T - 1 and mut != "omit_carry":
            dh = dh + bw["carry"][d]
        z, r, hh = (fw["gates"][d, :, t, q * H:(q + 1) * H] for q in range(3))
        qv = fw["qh"][d, :, t]
        hp = fw["hs"][:, prow + (1 if mut == "prow_plus_1" else 0), d * H:(d + 1) * H] if s > 0 else np.zeros((B, H), F)
        dz = dh * (hp - hh) * z * (one - z)
        dhh = dh * (one - z) * (one - hh * hh)
        dr = dhh * qv * r * (one - r)
        bw["dz"][d, :, t] = np.concatenate([dz, dr, dhh], 1)
        bw["dq"][d, :, t] = dhh * r
        bw["carry"][d] = dh * z


def emu_gru_bwd(U, fw, dh_seq, dh_last, upto=0, mut=None):
    dirs, B, T, H3 = fw["gates"].shape
    H = H3 // 3
    bw = dict(dz=np.zeros(fw["gates"].shape, F), dq=np.zeros((dirs, B, T, H), F), carry=np.zeros((dirs, B, H), F))
    for s in range(T - 1, upto - 1, -1):
        emu_gru_bwd_step(U, fw, dh_seq, dh_last, bw, s, mut)
    return bw


# ---------------------------------------------------------------------------------------------------- judging a stored state
def h_of(hs, dirs, H):
    """hseq [B, T+2, dirs H] -> h [dirs, B, T, H]"""
    T = hs.shape[1] - 2
    return np.stack([hs[:, 1:T + 1, d * H:(d + 1) * H] for d in range(dirs)])


def given(r, dat):
    """(dh_seq, dh_last) a row passes"""
    return (dat["dh_seq"] if r["dh"] in ("seq", "both") else None, dat["dh_last"] if r["dh"] in ("last", "both") else None)


def fwd_checks(r, dat, st):
    """[(name, stored values, reference pairs)] of a forward state st = dict(gates, c | qh, hs): every stored step from the
    stored state of its neighbour"""
    fam, H, dirs = fam_of(r), r["H"], r["dirs"]
    n = n_of(fam, H, True)
    h = h_of(st["hs"], dirs, H)
    if fam == "gru":
        ref = gru_fwd_ref(dat["U"], dat["brec"], dat["zg"], st["hs"], n)
        return [("gates", st["gates"], ref["gates"]), ("qh", st["qh"], ref["qh"]), ("h", h, ref["h"])]
    ref = lstm_fwd_ref(dat["U"], dat["zg"], st["hs"], st["c"], n)
    return [("gates", st["gates"], ref["gates"]), ("c", st["c"], ref["c"]), ("h", h, ref["h"])]


def bwd_checks(r, dat, st, bw):
    """[(name, values, reference pairs)] of backward's outputs bw = dict(dz, dq) given the forward state st"""
    fam, H = fam_of(r), r["H"]
    n = n_of(fam, H, False)
    dh_seq, dh_last = given(r, dat)
    if fam == "gru":
        dz, dq = gru_bwd_ref(dat["U"], st["gates"], st["qh"], st["hs"], dh_seq, dh_last, n)
        return [("dZx", bw["dz"], dz), ("dZrec_h", bw["dq"], dq)]
    return [("dZ", bw["dz"], lstm_bwd_ref(dat["U"], st["gates"], st["c"], dh_seq, dh_last, n))]


def ratio(got, ref):
    """|got - v| / e element by element (inf where got is not finite)"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref.v)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(err == 0.0, 0.0, err / ref.e)             # an exact value (a first step's qh is its bias) has e = 0
    return np.where(np.isfinite(got), q, np.inf)


# ---------------------------------------------------------------------------------------------------- 5. data
KINDS = ("normal", "offset")
SEED = 13                        # of the per-row draws


def _val(rng, kind, shape):
    z = rng.standard_normal(shape)
    return (z if kind == "normal" else 1.0 + 0.1 * z).astype(F)


def draw(fam, H, dirs, B, T, kind):
    """the inputs of a layer; a function of (family, H, B, T, kind) only, and direction 0 / row b do not depend on dirs / B
    beyond b, so that twins (the same shape through another path) and sub-batches see the same numbers"""
    ng = 3 if fam == "gru" else 4
    out = dict(U=[], brec=[])
    for d in range(2):
        rng = np.random.default_rng([ng, H, d, KINDS.index(kind)])
        mag = rng.uniform(0.5, 1.5, (H, ng * H)) if kind == "normal" else 1.0 + 0.1 * rng.standard_normal((H, ng * H))
        sign = np.where(rng.random((H, ng * H)) < 0.5, -1.0, 1.0)
        out["U"].append((sign * mag / math.sqrt(H)).astype(F))
        out["brec"].append(_val(rng, kind, ng * H))
    out["U"], out["brec"] = out["U"][:dirs], out["brec"][:dirs]
    zg = np.zeros((dirs, B, T, ng * H), F)
    dh_seq = np.zeros((B, T, dirs * H), F)
    dh_last = np.zeros((B, dirs * H), F)
    for b in range(B):
        rng = np.random.default_rng([ng, H, T, b, KINDS.index(kind), SEED])
        z = _val(rng, kind, (2, T, ng * H))
        s = _val(rng, kind, (T, 2, H))
        l = _val(rng, kind, (2, H))
        zg[:, b] = z[:dirs]
        dh_seq[b] = s[:, :dirs].reshape(T, dirs * H)
        dh_last[b] = l[:dirs].reshape(dirs * H)
    out.update(zg=zg, dh_seq=dh_seq, dh_last=dh_last)
    return out


# ---------------------------------------------------------------------------------------------------- PATHS
def _row(name, fam, H, dirs=2, B=3, T=3, shift=None, rs_extra=0, col=0, dh="seq", dh_wide=0, hlast=True, twin=None, **expect):
    """shift: buffer -> words its pointer is moved past a 16-byte aligned address (U0, U1, zg, hseq, qh).  rs_extra, col: rows
    of hseq are dirs H + rs_extra floats wide with the layer at column col (fused LSTM step only).  dh_wide: dh_seq's rows are
    that much wider, its batches one row longer.  dh: "seq" | "last" | "both".  expect: what the row is there for."""
    return dict(name=name, fam=fam, H=H, dirs=dirs, B=B, T=T, shift=dict(shift or {}), rs_extra=rs_extra, col=col, dh=dh,
                dh_wide=dh_wide, hlast=hlast, twin=twin, expect=expect)


def residues(r):
    """byte residues (mod 16) of the pointers the dispatch looks at"""
    s = r["shift"]
    res = {k: 4 * s.get(k, 0) % 16 for k in ("U0", "U1", "zg", "hseq", "qh")}
    res["hseq"] = (res["hseq"] + 4 * r["col"]) % 16
    if r["dirs"] == 1:
        res["U1"] = res["U0"]                                  # a.U[1] = U0
    return res


def h_rs(r):
    return r["dirs"] * r["H"] + r["rs_extra"]


STEP = []
# fwd_width 4: `H % 4 == 0 && h_rs % 4 == 0 && aligned_to(16, ..)`.  kpad 32 .. 256 in steps of 32 (H = 16 .. 256); H = 132: kpad
# 160 = one full prefetch group and a partial one of 1 block; 164: 2 blocks; 196: 3 blocks; 256: exactly one chunk, two groups
for _H in (16, 64, 68, 100, 132, 164, 196, 256):
    STEP.append(_row("w4_H%d" % _H, "step", _H, w=4, vec=True, kpads=[(_H + 31) & ~31]))
# fwd_width 2 through `H % 4`: H = 2 (mod 4); 250 is the model's own width
for _H in (18, 34, 66, 98, 130, 162, 194, 250):
    STEP.append(_row("w2_H%d" % _H, "step", _H, w=2, vec=True, kpads=[(_H + 31) & ~31]))
# fwd_width 2 at H = 16: each 16-byte condition fails alone while its 8-byte twin holds
STEP.append(_row("w2_H16_hseq8", "step", 16, shift={"hseq": 2}, twin="w4_H16", w=2, vec=True))
STEP.append(_row("w2_H16_U0_8", "step", 16, shift={"U0": 2}, twin="w4_H16", w=2, vec=False))
STEP.append(_row("w2_H16_U1_8", "step", 16, shift={"U1": 2}, twin="w4_H16", w=2, vec=False))
STEP.append(_row("w2_H16_rs2", "step", 16, rs_extra=2, twin="w4_H16", w=2, vec=True))
# fwd_width 1 through odd H; 255: kpad 256 with one dead k row; 257: a second chunk of klen 1
for _H in (1, 15, 17, 33, 65, 97, 129, 161, 193, 255, 257):
    STEP.append(_row("w1_H%d" % _H, "step", _H, w=1, vec=True,
                     kpads=[256, 32] if _H == 257 else [(_H + 31) & ~31]))
# fwd_width 1 at H = 16: each 8-byte condition fails alone
STEP.append(_row("w1_H16_U0_4", "step", 16, shift={"U0": 1}, twin="w4_H16", w=1, vec=False))
STEP.append(_row("w1_H16_U1_4", "step", 16, shift={"U1": 1}, twin="w4_H16", w=1, vec=False))
STEP.append(_row("w1_H16_hseq4", "step", 16, shift={"hseq": 1}, twin="w4_H16", w=1, vec=True))
STEP.append(_row("w1_H16_rs1", "step", 16, rs_extra=1, twin="w4_H16", w=1, vec=True))
# forward chunks of 256 rows (`kc += KCF`): 260 / 288 a second chunk of 4 / 32 rows through the float4 path; backward chunks of
# 1024 columns: 4H = 1020 (kpad 1024, 4 dead columns), 1024 (exactly one), 1028 (a second chunk of 4)
STEP.append(_row("chunk_H260", "step", 260, w=4, vec=True, kpads=[256, 32], bkpads=[1024, 32]))
STEP.append(_row("chunk_H288", "step", 288, w=4, vec=True, kpads=[256, 32], bkpads=[1024, 128]))
# backward `vec = aligned_to(16, U0, U1, zg)`: each pointer alone, at an odd and an even H (forward does not look at zg)
STEP.append(_row("bvec_H15_zg", "step", 15, shift={"zg": 1}, twin="w1_H15", w=1, vec=False))
STEP.append(_row("bvec_H15_U0", "step", 15, shift={"U0": 1}, twin="w1_H15", w=1, vec=False))
STEP.append(_row("bvec_H15_U1", "step", 15, shift={"U1": 1}, twin="w1_H15", w=1, vec=False))
STEP.append(_row("bvec_H16_zg", "step", 16, shift={"zg": 1}, twin="w4_H16", w=4, vec=False))
STEP.append(_row("bvec_H257_zg", "step", 257, shift={"zg": 2}, twin="w1_H257", w=1, vec=False, bkpads=[1024, 32]))
STEP.append(_row("bvec_H256_U1", "step", 256, shift={"U1": 3}, twin="w4_H256", w=1, vec=False, bkpads=[1024]))
# `a.dh_seq` / `a.dh_last && s == T - 1`; strides of dh_seq wider than dense; a column slice of a wider hseq
STEP.append(_row("dh_last_H17", "step", 17, dh="last", w=1, vec=True))
STEP.append(_row("dh_both_H16", "step", 16, dh="both", w=4, vec=True))
STEP.append(_row("dh_wide_H17", "step", 17, dh="both", dh_wide=5, twin=None, w=1, vec=True))
STEP.append(_row("slice_H16", "step", 16, rs_extra=64, col=32, twin="w4_H16", w=4, vec=True))
STEP.append(_row("slice_H250", "step", 250, rs_extra=1000, col=500, twin="w2_H250", w=2, vec=True))
# dirs = 1 with U1 = NULL (`a.U[1] = U0`); T = 1 (no product: `s > 0`, `s < T - 1` never true), T = 2, T = 4
STEP.append(_row("dirs1_H16", "step", 16, dirs=1, w=4, vec=True))
STEP.append(_row("dirs1_H17", "step", 17, dirs=1, dh="both", w=1, vec=True))
STEP.append(_row("T1_H16", "step", 16, T=1, dh="both", w=4, vec=True))
STEP.append(_row("T2_H34", "step", 34, T=2, w=2, vec=True))
STEP.append(_row("T4_H17", "step", 17, T=4, dh="both", w=1, vec=True))
# row tiles (`b < B`, `ra < B`: 64 rows per workgroup, 16 per wave) against unit slices (`u < H`: 16 per workgroup)
for _B in (1, 15, 16, 17, 63, 64, 65, 129):
    STEP.append(_row("tile_B%d_H16" % _B, "step", 16, B=_B, w=4, vec=True, grid=(cdiv(_B, 64), 1, 2)))
STEP.append(_row("tile_B65_H17", "step", 17, B=65, dh="both", w=1, vec=True, grid=(2, 2, 2)))
STEP.append(_row("tile_B17_H33", "step", 33, B=17, w=1, vec=True, grid=(1, 3, 2)))
STEP.append(_row("tile_B64_H15", "step", 15, B=64, w=1, vec=True, grid=(1, 1, 2)))
STEP.append(_row("tile_B1_H1", "step", 1, B=1, dh="both", w=1, vec=True, grid=(1, 1, 2)))

GRU = []
# `vec_ok = H % 4 == 0 && aligned_to(16, U0, U1, zg, hseq, qh)` true; 768 exactly one backward chunk per gate block, 772 a second
# chunk of 4 columns; 256 exactly one forward chunk
for _H in (16, 132, 256, 768, 772):
    GRU.append(_row("vec_H%d" % _H, "gru", _H, B=2 if _H > 700 else 3, T=2 if _H > 700 else 3, vec=True,
                    bkpads=[768, 32] if _H == 772 else [(_H + 31) & ~31]))
# false through `H % 4`; 767: kpad 768 with one dead column, 769: a second chunk of klen 1
for _H in (1, 15, 17, 33, 62, 767, 769):
    GRU.append(_row("sc_H%d" % _H, "gru", _H, B=2 if _H > 700 else 3, T=2 if _H > 700 else 3, vec=False,
                    bkpads=[768, 32] if _H == 769 else [(_H + 31) & ~31]))
# false through each of the five pointers alone
for _p in ("U0", "U1", "zg", "hseq", "qh"):
    GRU.append(_row("sc_H16_%s" % _p, "gru", 16, shift={_p: 1 if _p != "qh" else 2}, twin="vec_H16", vec=False))
# `a.hlast && s == T - 1` with hlast NULL; dh_seq / dh_last; dirs = 1 with U1 = b_rec1 = NULL; T = 1, 2, 4
GRU.append(_row("nohlast_H17", "gru", 17, hlast=False, twin="sc_H17", vec=False))
GRU.append(_row("dh_last_H16", "gru", 16, dh="last", vec=True))
GRU.append(_row("dh_both_H17", "gru", 17, dh="both", vec=False))
GRU.append(_row("dh_wide_H16", "gru", 16, dh="both", dh_wide=8, vec=True))
GRU.append(_row("dirs1_H16", "gru", 16, dirs=1, vec=True))
GRU.append(_row("dirs1_H15", "gru", 15, dirs=1, dh="both", vec=False))
GRU.append(_row("T1_H16", "gru", 16, T=1, dh="both", vec=True))
GRU.append(_row("T2_H33", "gru", 33, T=2, vec=False))
GRU.append(_row("T4_H17", "gru", 17, T=4, dh="both", vec=False))
for _B in (1, 15, 16, 17, 63, 64, 65, 129):
    GRU.append(_row("tile_B%d_H16" % _B, "gru", 16, B=_B, vec=True, grid=(cdiv(_B, 64), 1, 2)))
GRU.append(_row("tile_B65_H17", "gru", 17, B=65, dh="both", vec=False, grid=(2, 2, 2)))
GRU.append(_row("tile_B17_H33", "gru", 33, B=17, vec=False, grid=(1, 3, 2)))
GRU.append(_row("tile_B64_H15", "gru", 15, B=64, vec=False, grid=(1, 1, 2)))
GRU.append(_row("tile_B1_H1", "gru", 1, B=1, dh="both", vec=False, grid=(1, 1, 2)))

LSTM = []
# resident (`lidbox_lstm_resident_ok`): Hp = 16 .. 80; resident_lds crosses 64 KiB between Hp = 48 and Hp = 64 (allow_lds);
# RT = 1 with a workgroup of 4 rows holding 1, 3, 4 live rows and a second workgroup holding one (B = 5)
for _H, _B in ((1, 1), (16, 3), (17, 5), (48, 4), (64, 3), (65, 5), (80, 4)):
    LSTM.append(_row("res_H%d_B%d" % (_H, _B), "lstm", _H, B=_B, dh="both" if _H in (17, 80) else "seq", form="res", rt=1,
                     big_lds=pad16(_H) >= 64))
LSTM.append(_row("res_H16_B1", "lstm", 16, B=1, dh="last", form="res", rt=1))
LSTM.append(_row("res_dirs1_H17", "lstm", 17, dirs=1, form="res", rt=1))
LSTM.append(_row("res_T1_H16", "lstm", 16, T=1, dh="both", form="res", rt=1))
LSTM.append(_row("res_T4_H17", "lstm", 17, T=4, dh="both", form="res", rt=1))
# pick_rt: `ceil(B / (4 rt)) * dirs <= 256` first false at these B: the last workgroup (8 / 16 rows) holds ONE live row
LSTM.append(_row("res_rt2_d2_H17", "lstm", 17, B=513, form="res", rt=2, last_rows=1))
LSTM.append(_row("res_rt2_d1_H80", "lstm", 80, dirs=1, B=1025, dh="both", form="res", rt=2, last_rows=1))
LSTM.append(_row("res_rt4_d2_H80", "lstm", 80, B=1025, form="res", rt=4, last_rows=1))
LSTM.append(_row("res_rt4_d1_H17", "lstm", 17, dirs=1, B=2049, dh="both", form="res", rt=4, last_rows=1))
# stepped (`H > LSTM_RESIDENT_MAX_H`): GEMM + lstm_cell_{fwd,bwd}_kernel, 256 threads over dirs B H elements
for _H in (81, 100):
    for _B in (1, 17, 65):
        LSTM.append(_row("stp_H%d_B%d" % (_H, _B), "lstm", _H, B=_B, dh="both" if _B == 17 else "seq", form="stp"))
LSTM.append(_row("stp_dirs1_H81", "lstm", 81, dirs=1, dh="last", form="stp"))
LSTM.append(_row("stp_T1_H81", "lstm", 81, T=1, dh="both", form="stp"))

# lidbox_seq_avg_pool_fwd / _bwd: (B, T, C, pitched, alpha, accumulate).  `e >= B * C` forward at B C = 255 / 256 / 257 (one
# block less one thread, exactly one, a second block of one thread); `e >= B * T * C` backward at 255 / 256 / 257
POOL = [
    dict(name="f255", B=5, T=3, C=51, pitched=False, alpha=1.0, acc=0),
    dict(name="f256", B=4, T=2, C=64, pitched=True, alpha=0.25, acc=1),
    dict(name="f257", B=1, T=4, C=257, pitched=False, alpha=-1.5, acc=1),
    dict(name="T1", B=3, T=1, C=7, pitched=True, alpha=3.0, acc=0),
    dict(name="b255", B=3, T=5, C=17, pitched=True, alpha=0.5, acc=1),
    dict(name="b256", B=2, T=8, C=16, pitched=False, alpha=2.0, acc=0),
    dict(name="b257", B=1, T=1, C=257, pitched=True, alpha=1.0, acc=1),
]

PATHS = dict(step=STEP, gru=GRU, lstm=LSTM)


def fam_of(r):
    """the family of bounds and emulation a row runs under"""
    return r["fam"] if r["fam"] != "lstm" else lstm_form(r["H"])


def select(r):
    """what the restated dispatch selects for a row: kernels reached and the facts its comment names"""
    H, dirs, B = r["H"], r["dirs"], r["B"]
    p = residues(r)
    out = dict(kernels=set())
    if r["fam"] == "step":
        out["w"] = lstm_step_fwd_width(H, h_rs(r), p["U0"], p["U1"], p["hseq"])
        out["vec"] = lstm_step_bwd_vec(p["U0"], p["U1"], p["zg"])
        out["kpads"] = [c["kpad"] for c in chunk_plan(LstmStep, H, True)]
        out["bkpads"] = [c["kpad"] for c in chunk_plan(LstmStep, 4 * H, False)]
        out["last_group"] = [c["last"] for c in chunk_plan(LstmStep, H, True)]
        out["grid"] = step_grid(B, H, dirs)
        out["kernels"] = {("lstm_step_fwd_kernel", out["w"]), ("lstm_step_bwd_kernel", out["vec"])}
    elif r["fam"] == "gru":
        out["vec"] = gru_vec_ok(H, p["U0"], p["U1"], p["zg"], p["hseq"], p["qh"])
        out["kpads"] = [c["kpad"] for c in chunk_plan(GruStep, H, True)]
        out["bkpads"] = [c["kpad"] for c in chunk_plan(GruStep, H, False)]
        out["grid"] = step_grid(B, H, dirs)
        out["kernels"] = {("gru_fwd_step_kernel", out["vec"]), ("gru_bwd_step_kernel", out["vec"])}
    else:
        out["form"] = lstm_form(H)
        if out["form"] == "res":
            rt = out["rt"] = pick_rt(B, dirs)
            out["last_rows"] = B - (cdiv(B, 4 * rt) - 1) * 4 * rt
            out["big_lds"] = resident_lds(pad16(H), rt, False) > 64 * 1024
            out["kernels"] = {("lstm_resident_fwd_kernel", rt), ("lstm_resident_bwd_kernel", rt)}
        else:
            out["kernels"] = {("lstm_cell_fwd_kernel",), ("lstm_cell_bwd_kernel",)}
    return out


def reachable():
    """every kernel / instantiation of the recurrence files"""
    return ({("lstm_step_fwd_kernel", w) for w in (4, 2, 1)} | {("lstm_step_bwd_kernel", v) for v in (True, False)}
            | {(k, v) for k in ("gru_fwd_step_kernel", "gru_bwd_step_kernel") for v in (True, False)}
            | {(k, rt) for k in ("lstm_resident_fwd_kernel", "lstm_resident_bwd_kernel") for rt in (1, 2, 4)}
            | {("lstm_cell_fwd_kernel",), ("lstm_cell_bwd_kernel",), ("seq_avg_pool_fwd_kernel",), ("seq_avg_pool_bwd_kernel",)})
