"""float64 references of the three small kernels of the ByT5 G2P engine that the whole-model tests only see through logits
(phoonnx_amd/csrc/g2p.hip: g2p_attention_kernel, g2p_rmsnorm_kernel, g2p_argmax_kernel), and the input families that
tests/test_gpu_g2p_kernels.py runs through the hooks and tests/test_g2p_kernels_ref_cpu.py checks on the CPU: the same arrays.

An attention case is a dict of exactly what g2p_test_attention takes (phoonnx_amd.g2p.test_attention(**case)): flat q / out / k
/ v buffers with their strides.  The references read and write the same flat buffers through the same strides, so an element
the strides do not address keeps what `out` held."""
import numpy as np

from t5_oracle import relative_position_bucket

KMAX = 1024              # G2PModel::kMaxPos
LUT_ZERO = KMAX - 1
NUM_BUCKETS = 32
SENTINEL = np.float32(-777.25)
HEADS = 2


def bucket_lut(decoder):
    """bucket of (key position - query position) = d at index d + LUT_ZERO, as G2PModel::build fills bucket_enc / bucket_dec"""
    return relative_position_bucket(np.arange(-(KMAX - 1), KMAX), not decoder, NUM_BUCKETS, 128).astype(np.int32)


_LUTS = {}


def lut_of(kind):
    if kind not in _LUTS:
        _LUTS[kind] = bucket_lut(kind == "dec")
    return _LUTS[kind]


# ------------------------------------------------------------------------------------------------ references
def limits(c):
    """lim[b][i]: the number of keys column i of sequence b attends to"""
    nseq = c["cols"] // c["seg"]
    ipos = np.arange(c["seg"]) + c["q_off"]
    nk = np.full(nseq, c["Tk"]) if c["lens"] is None else np.asarray(c["lens"], np.int64)
    return np.minimum(ipos[None, :] + 1, nk[:, None]) if c["causal"] else np.repeat(nk[:, None], c["seg"], 1)


def owned(c):
    """flat indices of the (heads * dk) x cols elements of q / out the strides address, [channel, column]"""
    ch, col = np.arange(c["heads"] * c["dk"]), np.arange(c["cols"])
    return ch[:, None] * c["q_cs"] + col[None, :] * c["q_ts"]


def attention_ref(c, dtype=np.float64):
    """For every (column, head): scores q . k_j + bias[lut[j - (i + q_off) + LUT_ZERO]][h] over j < lim, softmax, the weighted
    sum of v - every operation in `dtype`.  Returns the `out` buffer (as `dtype`) with the owned elements written."""
    heads, dk, seg, q_cs, q_ts, kp, kv_bs = c["heads"], c["dk"], c["seg"], c["q_cs"], c["q_ts"], c["kp"], c["kv_bs"]
    q, k, v = (np.asarray(c[n]).reshape(-1) for n in ("q", "k", "v"))
    out = np.asarray(c["out"]).reshape(-1).astype(dtype)
    lim = limits(c)
    i = np.arange(seg)
    ipos = i + c["q_off"]
    for b in range(c["cols"] // seg):
        n = int(lim[b].max())      # (keys behind it belong to no query of this sequence: never read, whatever they hold)
        j = np.arange(n)
        col = b * seg + i
        for h in range(heads):
            ch = h * dk + np.arange(dk)
            at = ch[None, :] * q_cs + col[:, None] * q_ts                 # [seg, dk]
            kv = b * kv_bs + ch[:, None] * kp + j[None, :]                # [dk, n]
            s = q[at].astype(dtype) @ k[kv].astype(dtype)                 # [seg, n]
            if c["lut"] is not None:
                s = s + np.asarray(c["bias"])[c["lut"][j[None, :] - ipos[:, None] + LUT_ZERO], h].astype(dtype)
            s = np.where(j[None, :] < lim[b][:, None], s, np.dtype(dtype).type(-np.inf))
            e = np.exp(s - s.max(1, keepdims=True))
            out[at] = (e @ v[kv].astype(dtype).T) / e.sum(1, keepdims=True)   # (the sum, then one division: integer sums stay exact)
    return out


def rmsnorm_ref(x, g, y, T, eps, dtype=np.float64):
    """y[c][t] = x[c][t] * rsqrt(mean_c x[c][t]^2 + eps) * g[c] for t < T, in `dtype`; the other columns of y stay"""
    x, g, out = np.asarray(x)[:, :T].astype(dtype), np.asarray(g).astype(dtype), np.asarray(y).astype(dtype)
    f = np.dtype(dtype).type
    out[:, :T] = x * (f(1) / np.sqrt(np.mean(x * x, axis=0, keepdims=True, dtype=dtype) + f(eps))) * g[:, None]
    return out


def argmax_ref(row):
    """first maximum among the entries that are not NaN; 0 if there is none"""
    row = np.asarray(row)
    ok = np.flatnonzero(~np.isnan(row))
    return int(ok[np.argmax(row[ok])]) if ok.size else 0


# ------------------------------------------------------------------------------------------------ attention launches
TKS = (1, 2, 63, 64, 65, 255, 256, 257, 300, 513, 1023)
DK_TKS = {64: TKS, 16: TKS, 40: TKS, 20: (1, 65, 257), 128: (1, 65, 257)}
FORMS = ("enc", "pre_self", "pre_cross", "step_self_narrow", "step_self_wide", "step_cross_narrow", "step_cross_wide")


def prefill_groups(T):
    """The query columns a prefill form is run at, as (first column, count): all of a short prefix; of a long one the first
    column, 63 and 64, 255 and 256, and the last."""
    if T <= 65:
        return [(0, T)]
    return [(0, 1), (63, 2)] + ([(255, 2)] if T > 257 else []) + [(T - 1, 1)]


def seq_lens(Tk):
    return np.array([Tk, 1, min(Tk, 257), max(Tk - 1, 1)], np.int32)


def layouts(form, Tk, dk, heads=HEADS):
    """Every launch of `form` at Tk keys: the hook's arguments but for the data (q / out / k / v / bias)."""
    C = heads * dk
    base = dict(heads=heads, dk=dk, Tk=Tk, lens=None, lut=None, q_off=0, causal=False)
    if form == "enc":        # [C][4 S] activations; the four sequences' keys side by side in a row (here with a gap between them)
        S, kv_bs = Tk, Tk + 3
        kp = 3 * kv_bs + S + 5
        return [dict(base, q_cs=4 * S, q_ts=1, cols=4 * S, seg=S, lens=seq_lens(Tk), lut=lut_of("enc"), kp=kp, kv_bs=kv_bs, kv_n=C * kp)]
    if form in ("pre_self", "pre_cross"):   # [C][T] activations, one sequence, T = Tk; the columns of a group through q_off
        out = []
        for i0, n in prefill_groups(Tk):
            d = dict(base, q_cs=Tk, q_ts=1, cols=n, seg=n, q_off=0, kp=Tk + 5, kv_bs=0, kv_n=C * (Tk + 5), first_col=i0)
            if form == "pre_self":
                d.update(lut=lut_of("dec"), causal=True, q_off=i0)
            out.append(d)
        return out
    nb = 8 if form == "step_self_wide" else 4
    strides = dict(q_cs=1, q_ts=C) if form.endswith("narrow") else dict(q_cs=nb, q_ts=1)
    if form.startswith("step_self"):        # caches [NB][C][TM] (here with a gap between the sequences), Tk = t + 1
        TM = Tk + 6
        kv_bs = C * TM + 7
        return [dict(base, cols=nb, seg=1, lut=lut_of("dec"), causal=True, q_off=Tk - 1, kp=TM, kv_bs=kv_bs, kv_n=nb * kv_bs, **strides)]
    kv_bs = Tk + 3                          # step cross: the encoder's [C][4 S] keys, lens per sequence
    kp = 3 * kv_bs + Tk + 5
    return [dict(base, cols=nb, seg=1, lens=seq_lens(Tk), kp=kp, kv_bs=kv_bs, kv_n=C * kp, **strides)]


def _buffers(d):
    n = (d["heads"] * d["dk"] - 1) * d["q_cs"] + (d["cols"] - 1) * d["q_ts"] + 1
    return n, np.zeros(n, np.float32), np.full(n, SENTINEL, np.float32)


def _finish(d, q, k, v, bias):
    c = {key: val for key, val in d.items() if key not in ("kv_n", "first_col")}
    n, _, out = _buffers(d)
    c.update(q=np.ascontiguousarray(q, np.float32), out=out, k=np.ascontiguousarray(k, np.float32), v=np.ascontiguousarray(v, np.float32),
             bias=None if d["lut"] is None else np.ascontiguousarray(bias, np.float32))
    return c


def _seed(form, Tk, dk, n, salt):
    return [FORMS.index(form), Tk, dk, n, salt]


def random_cases(form, Tk, dk):
    """q, k standard normal scaled so that q . k has standard deviation 3, v standard normal, bias uniform in +-2"""
    out = []
    for n, d in enumerate(layouts(form, Tk, dk)):
        rng = np.random.default_rng(_seed(form, Tk, dk, n, 1))
        nq, _, _ = _buffers(d)
        s = np.sqrt(3.0) / dk ** 0.25
        out.append(_finish(d, rng.standard_normal(nq) * s, rng.standard_normal(d["kv_n"]) * s, rng.standard_normal(d["kv_n"]),
                           rng.uniform(-2, 2, (NUM_BUCKETS, d["heads"]))))
    return out


def poisoned(c):
    """The case with NaN in every key / value column no query of its sequence attends to (behind lens[b], behind the last
    causal position, the padding of a row) and in everything between the sequences' blocks."""
    lim = limits(c)
    keep = np.zeros(c["k"].size, bool)
    ch = np.arange(c["heads"] * c["dk"])
    for b in range(c["cols"] // c["seg"]):
        keep[(b * c["kv_bs"] + ch[:, None] * c["kp"] + np.arange(int(lim[b].max()))[None, :]).reshape(-1)] = True
    p = dict(c)
    p["k"], p["v"] = np.where(keep, c["k"], np.float32(np.nan)), np.where(keep, c["v"], np.float32(np.nan))
    return p


def _kv_index(d, b, ch, j):
    return b * d["kv_bs"] + ch * d["kp"] + j


def _ints(rng, n, lo=-8):
    """integers of magnitude 1 .. 8 (lo = -8: either sign; lo = 1: positive)"""
    a = rng.integers(1, 9, n).astype(np.float32)
    return a if lo > 0 else a * rng.choice(np.array([-1.0, 1.0], np.float32), n)


def _structured_v(d, rng, positive):
    """v: channel 0 of every head 1, channel 1 (if there is one) the key's index j (positive: j + 1), the rest integers of
    magnitude 1 .. 8 (positive: 1 .. 8)"""
    v = _ints(rng, d["kv_n"], 1 if positive else -8)
    j = np.arange(d["Tk"])
    for b in range(d["cols"] // d["seg"]):
        for h in range(d["heads"]):
            v[_kv_index(d, b, h * d["dk"], j)] = 1.0
            if d["dk"] > 1:
                v[_kv_index(d, b, h * d["dk"] + 1, j)] = j + 1 if positive else j
    return v


SELECTED_J = (0, 63, 64, 255, 256, 257, -1)   # (-1: lim - 1)


def selected_key_cases(form, Tk, dk):
    """q = 40 e_0 per head, k channel 0 one at key j* and zero elsewhere, no bias: the other keys weigh e^-40 = 4.2e-18 each, in
    all at most 1023 x 8 x 4.2e-18 = 3.5e-14 - below half an ulp of any |v| >= 1 and of the sum 1 - so out = v[:, j*] bit for
    bit.  j* per sequence: the wanted key, or the last one every query of the sequence attends to if that comes first.
    Yields (case, want): want[channel, column]."""
    out = []
    for n, d0 in enumerate(layouts(form, Tk, dk)):
        d = dict(d0, lut=None)
        lim = limits(d).min(1)     # per sequence: the keys EVERY one of its queries sees
        seen = set()
        for js in SELECTED_J:
            jb = tuple(int(min(js if js >= 0 else l - 1, l - 1)) for l in lim)
            if jb in seen:
                continue
            seen.add(jb)
            rng = np.random.default_rng(_seed(form, Tk, dk, n, 2))
            nq, q, _ = _buffers(d)
            own = owned(d)
            k, v = np.zeros(d["kv_n"], np.float32), _ints(rng, d["kv_n"])
            want = np.zeros(own.shape, np.float32)
            for h in range(d["heads"]):
                q[own[h * dk]] = 40.0
                for b, j in enumerate(jb):
                    k[_kv_index(d, b, h * dk, j)] = 1.0
            for b, j in enumerate(jb):
                want[:, b * d["seg"]:(b + 1) * d["seg"]] = v[_kv_index(d, b, np.arange(d["heads"] * dk), j)][:, None]
            out.append((_finish(d, q, k, v, None), want))
    return out


def uniform_cases(form, Tk, dk):
    """q = 0, no bias: every key of a query weighs 1 / lim.  v holds integers whose sums over any keys are integers below 2^24
    (exact in any order): out = sum / lim, channel 0 = 1, channel 1 = (lim - 1) / 2.  Yields (case, exact sums [channel, column]
    as float64, lim [column])."""
    out = []
    for n, d0 in enumerate(layouts(form, Tk, dk)):
        d = dict(d0, lut=None)
        rng = np.random.default_rng(_seed(form, Tk, dk, n, 3))
        nq, q, _ = _buffers(d)
        v = _structured_v(d, rng, False)
        c = _finish(d, q, rng.standard_normal(d["kv_n"]), v, None)
        out.append((c,) + _masked_sums(c, lambda b, h, j, ipos: np.ones((ipos.size, j.size), bool)))
    return out


def _masked_sums(c, select):
    """(sum of v over the selected keys [channel, column], their count [column]) - over all attended keys where none is
    selected; integer data: exact in float64"""
    lim = limits(c)
    dk, seg = c["dk"], c["seg"]
    sums, cnt = np.zeros((c["heads"] * dk, c["cols"])), np.zeros((c["heads"], c["cols"]), np.int64)
    ipos = np.arange(seg) + c["q_off"]
    for b in range(c["cols"] // seg):
        j = np.arange(int(lim[b].max()))
        att = j[None, :] < lim[b][:, None]
        for h in range(c["heads"]):
            sel = select(b, h, j, ipos) & att
            sel = np.where(sel.any(1, keepdims=True), sel, att)
            ch = h * dk + np.arange(dk)
            vv = c["v"][_kv_index(c, b, ch[:, None], j[None, :])].astype(np.float64)      # [dk, n]
            sums[h * dk:(h + 1) * dk, b * seg:(b + 1) * seg] = vv @ sel.T
            cnt[h, b * seg:(b + 1) * seg] = sel.sum(1)
    assert np.array_equal(sums, np.rint(sums)) and np.abs(sums).max() < 2 ** 24
    return sums, cnt


def bucket_cases(form, Tk, dk):
    """q = 0, bias[beta_h][h] = 40 and 0 elsewhere, beta_0 != beta_1 both among the buckets of the launch's (j - ipos): a key in
    bucket beta_h weighs 1, any other e^-40, so out = the mean of v over exactly the keys of that bucket (over all keys of a
    query that has none in it).  v: positive integers 1 .. 8 (no cancellation: what the other keys add, at most 3.5e-14, is
    far below an ulp of the sum), channel 1 = j + 1.  Yields (case, sums, counts [head, column])."""
    out = []
    for n, d in enumerate(layouts(form, Tk, dk)):
        assert d["lut"] is not None
        lim = limits(d)
        j = np.arange(int(lim[0].max()))
        present = np.unique(d["lut"][j - (d["q_off"] + 0) + LUT_ZERO])     # sequence 0, its first query
        if present.size < 2:
            continue
        beta = (int(present[present.size // 2]), int(present[-1])) if present[present.size // 2] != present[-1] else \
            (int(present[0]), int(present[-1]))
        beta = tuple(beta[h % 2] for h in range(d["heads"]))
        rng = np.random.default_rng(_seed(form, Tk, dk, n, 4))
        nq, q, _ = _buffers(d)
        bias = np.zeros((NUM_BUCKETS, d["heads"]), np.float32)
        for h, be in enumerate(beta):
            bias[be, h] = 40.0
        c = _finish(d, q, rng.standard_normal(d["kv_n"]), _structured_v(d, rng, True), bias)
        lut = d["lut"]
        out.append((c,) + _masked_sums(c, lambda b, h, j, ipos: lut[j[None, :] - ipos[:, None] + LUT_ZERO] == beta[h]))
    return out


def widened(c):
    """The case with heads of twice the width: the upper dk channels of q zero (the same scores), of k and v random."""
    dk, heads = c["dk"], c["heads"]
    assert c["q_ts"] == 1 or c["q_cs"] == 1
    C, C2 = heads * dk, 2 * heads * dk
    lo = (np.arange(heads)[:, None] * 2 * dk + np.arange(dk)[None, :]).reshape(-1)     # the wide channel of narrow channel ch
    w = dict(c, dk=2 * dk)
    rng = np.random.default_rng(c["Tk"] + 7)
    if c["q_cs"] == 1:       # [column][channel] vectors
        w["q_ts"] = C2
    nq = (C2 - 1) * w["q_cs"] + (c["cols"] - 1) * w["q_ts"] + 1
    q = np.zeros(nq, np.float32)
    own_n, own_w = owned(c), owned(w)
    q[own_w[lo]] = c["q"][own_n]
    w["q"], w["out"] = q, np.full(nq, SENTINEL, np.float32)
    nseq = c["cols"] // c["seg"]
    # k / v: the same row pitch and sequence stride where rows of sequences share a row; a cache holds twice the rows
    cache = c["kv_bs"] >= C * c["kp"]
    w["kv_bs"] = c["kv_bs"] + C * c["kp"] if cache else c["kv_bs"]
    size = nseq * w["kv_bs"] if cache else C2 * c["kp"]
    for name in ("k", "v"):
        a = rng.standard_normal(size).astype(np.float32)
        j = np.arange(c["Tk"])
        for b in range(nseq):
            a[_kv_index(w, b, lo[:, None], j[None, :])] = c[name][_kv_index(c, b, np.arange(C)[:, None], j[None, :])]
        w[name] = a
    return w, lo


# ------------------------------------------------------------------------------------------------ RMS norm, argmax
RMS_C = (1, 8, 255, 256, 257, 1472)
RMS_T = (1, 3, 40)


def rms_case(C, T, exact=False):
    """x [C, T + 3], g [C], y [C, T + 5] filled with the sentinel, eps.  exact: x = +-1, g integers, eps 0 (mean x^2 = 1)"""
    rng = np.random.default_rng([C, T, int(exact)])
    if exact:
        x = rng.choice(np.array([-1.0, 1.0], np.float32), (C, T + 3))
        g, eps = _ints(rng, C), 0.0
    else:
        x = (rng.standard_normal((C, T + 3)) * rng.uniform(0.3, 3.0, (1, T + 3))).astype(np.float32)
        g, eps = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32), 1e-6
    return x, g, np.full((C, T + 5), SENTINEL, np.float32), eps


ARGMAX_V = (1, 255, 256, 257, 384, 1001)
ARGMAX_NB = (1, 4, 8, 64)


def argmax_layout(wide, V, NB, t=0):
    """(pitch, lb, size, flat index [NB, V]) of the two logits layouts: wide [V][NB] (pitch NB, lb 1), narrow [NB][V] (pitch 1, lb V)"""
    pitch, lb = (NB, 1) if wide else (1, V)
    at = np.arange(NB)[:, None] * lb + np.arange(V)[None, :] * pitch + t
    return pitch, lb, (NB - 1) * lb + (V - 1) * pitch + t + 1, at


def argmax_rows(V, NB):
    """NB rows of V logits and what each shows: the maximum placed at 0 / 255 / 256 / V - 1, equal maxima (the lower index wins),
    -0.0 against +0.0, all -inf, all NaN, NaNs around finite values."""
    rng = np.random.default_rng([V, NB])
    rows = rng.standard_normal((NB, V)).astype(np.float32)
    kinds = []
    places = [p for p in (0, 255, 256, V - 1) if p < V]
    pairs = [p for p in ((5, 300), (255, 256), (0, V - 1)) if p[1] < V and p[0] != p[1]]
    for b in range(NB):
        kind = b % 8
        if kind == 0:
            rows[b, places[(b // 8) % len(places)]] = 9.0
        elif kind == 1 and pairs:
            lo, hi = pairs[(b // 8) % len(pairs)]
            rows[b, hi] = rows[b, lo] = 9.0
        elif kind == 2:
            rows[b] = -0.0
            rows[b, V - 1] = 0.0        # +0.0 == -0.0: index 0 wins
        elif kind == 3:
            rows[b] = -np.inf
        elif kind == 4:
            rows[b] = np.nan
        elif kind == 5:
            rows[b, ::2] = np.nan       # NaN at 0, 2, ...: the first maximum among the others
            if V > 1:
                rows[b, 1::2][-1] = 7.0
                if V > 3:
                    rows[b, 1] = 7.0
        elif kind == 6:
            rows[b, places[(b // 8 + 1) % len(places)]] = 9.0
        kinds.append(kind)
    return rows, kinds
