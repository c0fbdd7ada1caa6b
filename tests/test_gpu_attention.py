"""The text encoder's two attention kernels by value, instantiation by instantiation: attention_relpos16_kernel<DKS, NS, QT>
(csrc/attention16.hip.hpp: f16x3 products, LDS-DMA staging NS stages deep, 64 QT queries per workgroup, 32 keys per block) and
the fp32-MFMA attention_relpos_kernel<DKB, KH> (csrc/kernels.hip.hpp: 128 queries per workgroup, KH key halves), each launch
through session.test_attention_form, which names the form (fp32 output, operand planes, or both - the pipeline's attention16
launch writes planes only) and the instantiation, and returns the device buffers whole (0xff bytes where the launch wrote
nothing), the range guard's peak and the name of the instantiation started.

The reference is tests/attention_ref.py in float64.  Against it (groups a, c, d, e) the fp32 output is held, per case, to
8 x the largest error of the same formula evaluated in float32 NumPy on the same input, at least 2^-22 max|want|, and nowhere
above the tolerances of the first attention tests (2e-5 + 1e-4 |ref|; 1e-4 + 1e-4 |ref| for sharp softmaxes): see
attention_ref.tolerance for what the 8 covers.  Everything else needs no tolerance: instantiations against <3, 2, 1> (b),
forms against each other, zero columns, sentinels, the peak (c) and independence from padding, row pitch and batch
neighbours (f) are bit for bit.  The planes are held to the split's own 3e-7 relative to the fp32 value they copy.

Every figure is printed in front of its assertion; WORST keeps the largest ratio per (group, check), REACHED the instantiations
started, both printed at the end.

Measured on an MI355X (profiles/attention_tests/README.md has the table): the largest error is 0.48 x the bound (attention16,
dk 96, group a and the one-hot band inputs), 0.17 x for the fp32 kernel; the planes reach 0.40 x their 3e-7; every bit-for-bit
claim holds, QT = 2 included.
"""
import numpy as np
import pytest

import attention_ref as ar

pytestmark = pytest.mark.gpu

WORST = {}
REACHED = set()
A16_L = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 161, 193)
F32_L = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 161)
A16_INST = {32: [(3, 1)], 64: [(3, 1)], 96: [(2, 1), (3, 1), (4, 1), (2, 2), (3, 2)]}   # (NS, QT) per head width
ALL_KERNELS = sorted([f"attention_relpos16_kernel<{dk // 32}, {ns}, {qt}>" for dk, v in A16_INST.items() for ns, qt in v] +
                     [f"attention_relpos_kernel<{dkb}, {kh}>" for dkb in (1, 2, 3, 4) for kh in (1, 2)])


def _note(group, what, ratio, kernel):
    key = (group, what)
    if key not in WORST or ratio > WORST[key][0]:
        WORST[key] = (ratio, kernel)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\nWORST ratio per (group, check):")
    for (group, what), (ratio, kernel) in sorted(WORST.items()):
        print(f"  [{group}] {what}: {ratio:.3f} x bound ({kernel})")
    print("instantiations reached:")
    for k in sorted(REACHED):
        print("  " + k)
    print("instantiations not reached: " + (", ".join(k for k in ALL_KERNELS if k not in REACHED) or "none"))


class Case:
    """one input, its float64 reference and the per-element bound, computed once and shared by every launch of that input"""

    def __init__(self, qkv, heads, rk, rv, lens, sharp=False):
        self.qkv, self.heads, self.rk, self.rv = qkv, heads, rk, rv
        self.lens = np.asarray(lens, np.int64)
        self.B, self.T = qkv.shape[0], qkv.shape[2]
        self.C = qkv.shape[1] // 3
        self.dk = self.C // heads
        self.L = [int(min(l, self.T)) for l in self.lens]
        self.sharp = sharp
        self._ref = None

    def ref(self):
        if self._ref is None:
            want = ar.attention_ref(self.qkv, self.heads, self.rk, self.rv, self.lens)
            f32 = ar.attention_ref_f32(self.qkv, self.heads, self.rk, self.rv, self.lens)
            self._ref = (want,) + ar.tolerance(want, f32, self.sharp)
        return self._ref


def name16(dk, ns=0, qt=0):
    d_ns, d_qt = A16_INST[dk][0]
    return f"attention_relpos16_kernel<{dk // 32}, {ns or d_ns}, {qt or d_qt}>"


def name32(dk, kh):
    return f"attention_relpos_kernel<{(dk + 31) // 32}, {kh}>"


def launch(case, kernel, want_out=True, want_planes=True, expect=None, **kw):
    from phoonnx_amd.session import test_attention_form
    r = test_attention_form(case.qkv, case.heads, case.rk, case.rv, case.lens, kernel=kernel, want_out=want_out,
                            want_planes=want_planes, **kw)
    REACHED.add(r["kernel"])
    if expect is not None:
        assert r["kernel"] == expect, (r["kernel"], expect)
    r["want_out"], r["want_planes"] = want_out, want_planes
    return r


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_value(group, case, r, what="out", key=None):
    """the fp32 output against float64 on the valid queries, by the tolerance rule (`key`: the WORST row, default `what`)"""
    want, bound, scalar = case.ref()
    worst, worst_s = 0.0, 0.0
    for b, L in enumerate(case.L):
        if L == 0:
            continue
        err = np.abs(r["out"][b, :, :L].astype(np.float64) - want[b, :, :L])
        worst = max(worst, float((err / bound[b, :, :L]).max()))
        worst_s = max(worst_s, float(err.max()) / scalar)
    print(f"[{group}] {r['kernel']} dk {case.dk} T {case.T} lens {case.L[:4]}: {what} {worst:.3f} x bound "
          f"({worst_s:.3f} x the bound before its ceiling, {scalar:.2e})")
    _note(group, (key or what) + " vs float64", worst, r["kernel"])
    assert np.isfinite(worst) and worst <= 1.0, (r["kernel"], case.dk, case.T, case.L, worst)


def check_layout(group, case, r, out_of=None):
    """what needs no tolerance: zeros in the columns [len, T) of everything written, nothing written where nothing was asked
    for, the third plane slot untouched, every owned element written, the peak exactly max|out| (0 without planes), and the
    planes as the split of the fp32 output (3e-7 relative, the split's own figure).  out_of: the launch whose fp32 output a
    planes-only launch is held to."""
    out, pl = r["out"], r["planes"]
    sent32 = _bits32(out) == 0xFFFFFFFF
    if r["want_out"]:
        assert not sent32.any(), f"{int(sent32.sum())} fp32 outputs were never written"
        for b, L in enumerate(case.L):
            assert not _bits32(out[b, :, L:]).any(), "non-zero bits behind len in out"
    else:
        assert sent32.all(), "the launch wrote an fp32 output nobody asked for"
    if pl is not None:
        assert (pl[:, 2] == 0xFFFF).all(), "the third plane slot was written"
        if r["want_planes"]:
            assert not (pl[:, :2] == 0xFFFF).any(), "plane cells were never written"
            for b, L in enumerate(case.L):
                assert not pl[b, :2, :, L:].any(), "non-zero bits behind len in the planes"
        else:
            assert (pl == 0xFFFF).all(), "the launch wrote planes nobody asked for"
    src = r if r["want_out"] else out_of
    if r["want_planes"]:
        val = ar.planes_value(pl)
        o64 = src["out"].astype(np.float64)
        ratio = float((np.abs(val - o64) / (1e-9 + 3e-7 * np.abs(o64))).max())
        peak_want = float(np.abs(src["out"]).max())
        print(f"[{group}] {r['kernel']}: planes {ratio:.3f} x (1e-9 + 3e-7 |out|); peak {r['peak']!r} against max|out| {peak_want!r}")
        _note(group, "planes vs out", ratio, r["kernel"])
        assert ratio <= 1.0
        assert np.float32(r["peak"]) == np.float32(peak_want)
    else:
        print(f"[{group}] {r['kernel']}: no planes, peak {r['peak']!r}")
        assert r["peak"] == 0.0


def same_bits(a, b, what):
    assert a["out"].shape == b["out"].shape
    d = int((_bits32(a["out"]) != _bits32(b["out"])).sum())
    dp = 0 if a["planes"] is None or b["planes"] is None else int((a["planes"] != b["planes"]).sum())
    md = float(np.abs(a["out"].astype(np.float64) - b["out"].astype(np.float64)).max()) if d else 0.0
    print(f"{what}: {a['kernel']} against {b['kernel']}: {d} fp32 outputs and {dp} plane words differ (largest difference {md:.3e})")
    assert d == 0 and dp == 0, what


def valid_bits_equal(case_a, ra, case_b, rb, what, rows=None):
    """the valid outputs of two launches whose inputs agree on the valid columns: bit for bit, out and planes"""
    rows = rows if rows is not None else [(b, b) for b in range(case_a.B)]
    bad = 0
    for ba, bb in rows:
        L = case_a.L[ba]
        assert L == case_b.L[bb]
        bad += int((_bits32(ra["out"][ba, :, :L]) != _bits32(rb["out"][bb, :, :L])).sum())
        if ra["planes"] is not None and rb["planes"] is not None and ra["want_planes"] and rb["want_planes"]:
            bad += int((ra["planes"][ba, :2, :, :L] != rb["planes"][bb, :2, :, :L]).sum())
    print(f"{what}: {ra['kernel']} T {case_a.T} against T {case_b.T}: {bad} valid words differ")
    assert bad == 0, what


def has_planes(kernel, dk):
    return kernel == 16 or dk % 8 == 0


# ------------------------------------------------------------------ (a) lengths

def _length_case(dk, L, T):
    qkv, rk, rv = ar.random_case(1000 * dk + L, 2, 2, dk, T)
    return Case(qkv, 2, rk, rv, [L, (L + 1) // 2])


@pytest.mark.parametrize("dk", [32, 64, 96])
def test_a_lengths_attention16(dk):
    """one key block, the block seams (31 / 32 / 33 ...), the second query tile (65), NS - 1 prefetched blocks and more, the
    stage ring going round (161, 193: six and seven blocks over two or three stages), each with T = L and with a ragged pitch"""
    for L in A16_L:
        for T in (L, L + 11):
            case = _length_case(dk, L, T)
            r = launch(case, 16, expect=name16(dk))
            check_value("a", case, r)
            check_layout("a", case, r)


@pytest.mark.parametrize("kh", [1, 2])
@pytest.mark.parametrize("dk", [8, 12, 16, 48, 96, 100, 104, 128])
def test_a_lengths_fp32_kernel(dk, kh):
    """DKB 1 - 4, whole (`full`) and partial last channel blocks, with planes wherever the head width allows them (12 and 100
    do not), one and two key halves (the halves differ from 33 keys on; from 65 on both hold whole blocks).  DKB = 4 holds
    76,816 bytes of static LDS with two halves (35,344 with one), read from the build's resource remarks: under the 163,840 a
    workgroup may declare on gfx950."""
    for n, L in enumerate(F32_L):
        T = L + (11 if n % 2 else 0)
        case = _length_case(dk, L, T)
        r = launch(case, 32, want_planes=has_planes(32, dk), kh=kh, expect=name32(dk, kh))
        check_value("a", case, r)
        check_layout("a", case, r)


# ------------------------------------------------------------------ (b) instantiations

@pytest.fixture(scope="module")
def b_base():
    """the dk = 96 inputs of (a) - every length with T = L and with T = L + 11 - plus one ragged batch, each launched once on
    <3, 2, 1> and held to float64 and to the layout checks: [(tag, case, launch)]"""
    cases = [(f"L{L} T{T}", _length_case(96, L, T)) for L in A16_L for T in (L, L + 11)]
    qkv, rk, rv = ar.random_case(4242, 5, 2, 96, 200)
    cases.append(("ragged", Case(qkv, 2, rk, rv, [200, 1, 130, 64, 65])))
    out = []
    for tag, case in cases:
        base = launch(case, 16, ns=2, qt=1, expect=name16(96, 2, 1))
        check_value("b", case, base)
        check_layout("b", case, base)
        out.append((tag, case, base))
    return out


@pytest.mark.parametrize("ns,qt", [(3, 1), (4, 1), (2, 2), (3, 2)])
def test_b_attention16_instantiations_are_bit_identical(b_base, ns, qt):
    """Stage depth only changes WHICH LDS stage a key block waits in and how many blocks are in flight; the blocks are consumed
    in the same order by the same MFMA sequence.  A second query tile per wave gives every 16-query tile its own accumulators,
    softmax statistics and rescale decision (the ballot spans the wave, which holds exactly one tile's 16 queries in either
    form): no sum and no order changes.  So every instantiation must equal <3, 2, 1> bit for bit, out, planes and peak."""
    assert len(b_base) == 2 * len(A16_L) + 1
    for tag, case, base in b_base:
        r = launch(case, 16, ns=ns, qt=qt, expect=name16(96, ns, qt))
        same_bits(r, base, f"[b] {tag}")
        assert np.float32(r["peak"]) == np.float32(base["peak"])
        check_layout("b", case, r)


# ------------------------------------------------------------------ (c) forms

def _form_cases(kernel):
    if kernel == 16:
        return [(dk, L, inst) for dk in (32, 96) for L in (33, 65, 129) for inst in ([{}] if dk == 32 else [{}, {"ns": 3, "qt": 2}])]
    return [(dk, L, {"kh": kh}) for dk in (16, 96, 128) for L in (33, 129) for kh in (1, 2)]


@pytest.mark.parametrize("kernel", [16, 32])
def test_c_forms(kernel):
    """both outputs, the fp32 output alone, the planes alone (attention16: what the pipeline launches): the planes of "planes
    only" are those of "both", the fp32 output is the same wherever it is written, nothing else is touched, and the range guard
    reports max|out| exactly - 0 where no planes are written"""
    for dk, L, inst in _form_cases(kernel):
        case = _length_case(dk, L, L + 11)
        both = launch(case, kernel, **inst)
        check_value("c", case, both)
        check_layout("c", case, both)
        only_out = launch(case, kernel, want_planes=False, **inst)
        check_layout("c", case, only_out)
        assert (_bits32(only_out["out"]) == _bits32(both["out"])).all()
        if kernel == 16:
            only_pl = launch(case, kernel, want_out=False, **inst)
            check_layout("c", case, only_pl, out_of=both)
            assert (only_pl["planes"] == both["planes"]).all()
            assert np.float32(only_pl["peak"]) == np.float32(both["peak"])
            # q | k | v planes split on the host and handed in: the launch the pipeline makes from its conv's planes
            given = launch(case, kernel, want_out=False, qkv_planes=ar.split_planes(case.qkv), **inst)
            d = int((given["planes"] != both["planes"]).sum())
            print(f"[c] planes given by the caller against the device split: {d} plane words differ")
            assert d == 0


# ------------------------------------------------------------------ (d) the band

def _band_lengths(w):
    return sorted({L for L in (1, 2, w, w + 1, 33, 65) if L >= 1})


BAND_KERNELS = [(16, 32, {}), (16, 96, {"ns": 3, "qt": 2}), (32, 16, {"kh": 2}), (32, 104, {"kh": 1})]


@pytest.mark.parametrize("window", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("kernel,dk,inst", BAND_KERNELS)
def test_d_band_one_hot(kernel, dk, inst, window):
    """k = 0 and one relative-key logit of 64 per query: the output is V[:, i + m* - w] + E_v[m*], or the uniform average where
    that key does not exist (both ends of the utterance, every m*, utterances shorter than the band); V = 0 leaves the
    relative-value term alone.  A band index off by one, or a wrong end test, moves these outputs by O(|V|, |E_v|) = O(1)."""
    rng = np.random.default_rng(100 * dk + window)
    for L in _band_lengths(window):
        for m_star in range(2 * window + 1):
            for v_zero in (False, True):
                qkv, rk, rv, lens = ar.band_one_hot(dk, 2, window, m_star, L, L + 5, rng, v_zero=v_zero)
                case = Case(qkv, 2, rk, rv, lens, sharp=True)
                r = launch(case, kernel, want_planes=has_planes(kernel, dk), **inst)
                check_value("d", case, r, what=f"one-hot m* {m_star}" + (" V=0" if v_zero else ""),
                            key="one-hot V=0" if v_zero else "one-hot")
                check_layout("d", case, r)


@pytest.mark.parametrize("window", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("kernel,dk,inst", BAND_KERNELS)
def test_d_band_unit_scale_embeddings(kernel, dk, inst, window):
    """random inputs with E_k, E_v at unit scale (a trained voice holds them at dk^-0.5, where one wrong band entry hides in the
    tolerance), every window the engine accepts, two utterances of which one is shorter than the band"""
    qkv, rk, rv = ar.random_case(77 + window, 2, 2, dk, 76, window, rel_scale=1.0)
    case = Case(qkv, 2, rk, rv, [65, 3], sharp=True)
    r = launch(case, kernel, want_planes=has_planes(kernel, dk), **inst)
    check_value("d", case, r, what="unit-scale band")
    check_layout("d", case, r)


# ------------------------------------------------------------------ (e) rescale

@pytest.mark.parametrize("kind", ar.RESCALE_KINDS)
@pytest.mark.parametrize("kernel,dk,inst", [(16, 32, {}), (16, 64, {}), (16, 96, {}), (16, 96, {"ns": 4}), (16, 96, {"ns": 3, "qt": 2}),
                                            (32, 48, {"kh": 1}), (32, 48, {"kh": 2}), (32, 128, {"kh": 2})])
def test_e_rescale(kernel, dk, inst, kind):
    """the running maximum moving in every key block, never, inside the band, in the last, partly masked block (with larger
    logits still behind len), and late on top of sharp logits: six key blocks (161 keys), so both key halves of the fp32 kernel
    hold three and their states meet with different maxima"""
    qkv, rk, rv, lens = ar.rescale_case(kind, 5, 2, dk, 161, 172)
    case = Case(qkv, 2, rk, rv, lens, sharp=True)
    r = launch(case, kernel, want_planes=has_planes(kernel, dk), **inst)
    check_value("e", case, r, what=kind)
    check_layout("e", case, r)


# ------------------------------------------------------------------ (f) independence

INDEP_KERNELS = [(16, 32, {}), (16, 64, {}), (16, 96, {}), (16, 96, {"ns": 3, "qt": 2}), (32, 16, {"kh": 1}), (32, 16, {"kh": 2}),
                 (32, 100, {"kh": 2}), (32, 128, {"kh": 1}), (32, 128, {"kh": 2})]


def _with_padding(qkv, lens, fill):
    out = np.array(qkv, copy=True)
    for b, L in enumerate(lens):
        pad = out[b, :, L:]
        if fill == "zeros":
            pad[...] = 0.0
        else:  # +-1000: finite, inside fp16's range, and far above any valid logit
            sign = np.where((np.arange(pad.shape[0])[:, None] + np.arange(pad.shape[1])[None, :]) % 2 == 0, 1.0, -1.0)
            pad[...] = 1000.0 * sign
    return out


@pytest.mark.parametrize("kernel,dk,inst", INDEP_KERNELS)
def test_f_valid_outputs_do_not_depend_on_what_lies_behind_len(kernel, dk, inst):
    """columns >= len of q, k and v at +-1000 against zeros there: the valid outputs keep every bit (masked keys carry weight
    exactly 0, padded queries are never stored), and the columns behind len stay zero"""
    for lens, T in (([40, 17], 64), ([65, 1], 76), ([129, 97], 140)):
        qkv, rk, rv = ar.random_case(dk + T, 2, 2, dk, T)
        ca = Case(_with_padding(qkv, lens, "zeros"), 2, rk, rv, lens)
        cb = Case(_with_padding(qkv, lens, "big"), 2, rk, rv, lens)
        pl = has_planes(kernel, dk)
        ra, rb = launch(ca, kernel, want_planes=pl, **inst), launch(cb, kernel, want_planes=pl, **inst)
        valid_bits_equal(ca, ra, cb, rb, f"[f] padding +-1000 lens {lens}")
        check_layout("f", cb, rb)
        check_value("f", ca, ra)


@pytest.mark.parametrize("kernel,dk,inst", INDEP_KERNELS)
def test_f_valid_outputs_do_not_depend_on_the_row_pitch(kernel, dk, inst):
    """T = L against L + 11 and L + 70 (another query tile, other workgroup ids, noise behind len), and len > T as len = T"""
    for L in (33, 65, 129):
        qkv, rk, rv = ar.random_case(7 * dk + L, 2, 2, dk, L + 70)
        lens = [L, L - 20]
        pl = has_planes(kernel, dk)
        cases = [Case(np.ascontiguousarray(qkv[:, :, :T]), 2, rk, rv, lens) for T in (L, L + 11, L + 70)]
        rs = [launch(c, kernel, want_planes=pl, **inst) for c in cases]
        for c, r in zip(cases[1:], rs[1:]):
            valid_bits_equal(cases[0], rs[0], c, r, f"[f] row pitch L {L}")
            check_layout("f", c, r)
        over = Case(cases[0].qkv, 2, rk, rv, [L + 5, L - 20])
        ro = launch(over, kernel, want_planes=pl, **inst)
        same_bits(ro, rs[0], f"[f] len {L + 5} > T {L}")


@pytest.mark.parametrize("B,heads", [(1, 1), (3, 2), (4, 2), (9, 1), (17, 1)])
@pytest.mark.parametrize("kernel,dk,inst", [(16, 32, {}), (16, 96, {}), (16, 96, {"ns": 3, "qt": 2}), (32, 16, {"kh": 2}), (32, 104, {"kh": 1}),
                                            (32, 128, {"kh": 2})])
def test_f_rows_of_a_ragged_batch_equal_the_rows_alone(kernel, dk, inst, B, heads):
    """B n_heads = 1, 6, 8, 9, 17 (attention16 deals workgroup ids to (XCD, pair, tile): below, at and above one round of eight),
    rows of length 1, rows whose later query tiles are all padding: each row of the batch equals the same row launched alone"""
    T = 150
    lens = [(T, 1, 97, 64, 33, 150, 2, 129, 65)[b % 9] for b in range(B)]
    qkv, rk, rv = ar.random_case(B * 31 + dk, B, heads, dk, T)
    pl = has_planes(kernel, dk)
    batch = Case(qkv, heads, rk, rv, lens)
    rb = launch(batch, kernel, want_planes=pl, **inst)
    check_layout("f", batch, rb)
    bad = 0
    for b in range(B):
        one = Case(np.ascontiguousarray(qkv[b:b + 1]), heads, rk, rv, lens[b:b + 1])
        r1 = launch(one, kernel, want_planes=pl, **inst)
        bad += int((_bits32(r1["out"][0]) != _bits32(rb["out"][b])).sum())
        if pl:
            bad += int((r1["planes"][0] != rb["planes"][b]).sum())
    print(f"[f] {rb['kernel']} B {B} x {heads} heads: {bad} words differ between the batch's rows and the rows alone")
    assert bad == 0


# ------------------------------------------------------------------ (g) refusals

def _raises(match, fn, *a, **kw):
    from phoonnx_amd.session import SessionError
    with pytest.raises(SessionError, match=match) as e:
        fn(*a, **kw)
    print(f"[g] refused: {e.value}")


def test_g_refusals():
    """a head wider than the widest instantiation covers (it would lose channels 128.. without an error), a head width
    attention16 is not compiled for, a window beyond the nine relative positions the kernels hold, and every (ns, qt, kh) without
    an instantiation - refused, never rounded to a neighbour"""
    from phoonnx_amd.session import test_attention, test_attention16, test_attention_form
    lens = [20]
    qkv, rk, rv = ar.random_case(1, 1, 1, 160, 20)
    _raises("head width 160", test_attention, qkv, 1, rk, rv, lens)
    _raises("head width 160", test_attention16, qkv, 1, rk, rv, lens, kernel=0)
    _raises("head width 160", test_attention_form, qkv, 1, rk, rv, lens, kernel=32)
    _raises("head width 160", test_attention_form, qkv, 1, rk, rv, lens, kernel=16)
    qkv, rk, rv = ar.random_case(2, 1, 2, 48, 20)
    _raises("32, 64 or 96", test_attention_form, qkv, 2, rk, rv, lens, kernel=16)
    _raises("32, 64 or 96", test_attention16, qkv, 2, rk, rv, lens, kernel=1)
    for dk in (32, 48):
        qkv, rk, rv = ar.random_case(3, 1, 2, dk, 20, window=5)
        _raises("window", test_attention_form, qkv, 2, rk, rv, lens, kernel=32)
        _raises("attention", test_attention, qkv, 2, rk, rv, lens)
        if dk == 32:
            _raises("window", test_attention_form, qkv, 2, rk, rv, lens, kernel=16)
            _raises("attention", test_attention16, qkv, 2, rk, rv, lens, kernel=1)
    qkv, rk, rv = ar.random_case(4, 1, 2, 32, 20)
    for kw in (dict(ns=2), dict(ns=4), dict(qt=2), dict(kh=1)):
        _raises("instantiation|key halves", test_attention_form, qkv, 2, rk, rv, lens, kernel=16, **kw)
    for kw in (dict(kh=3), dict(ns=2), dict(qt=1), dict(want_out=False)):
        _raises("instantiation|stages|always writes", test_attention_form, qkv, 2, rk, rv, lens, kernel=32, **kw)
    _raises("neither output", test_attention_form, qkv, 2, rk, rv, lens, kernel=16, want_out=False, want_planes=False)
    _raises("kernel must be", test_attention_form, qkv, 2, rk, rv, lens, kernel=1)
    qkv, rk, rv = ar.random_case(5, 1, 2, 96, 20)
    for kw in (dict(ns=4, qt=2), dict(ns=5), dict(ns=1), dict(qt=3)):
        _raises("instantiation", test_attention_form, qkv, 2, rk, rv, lens, kernel=16, **kw)
    qkv, rk, rv = ar.random_case(6, 1, 2, 12, 20)
    _raises("multiple of 8", test_attention_form, qkv, 2, rk, rv, lens, kernel=32, want_planes=True)


def test_z_every_instantiation_starts_under_its_own_name():
    """the seven attention16 instantiations and DKB 1 - 4 x KH 1 - 2 of the fp32 kernel, one small launch each: the hook's
    arguments reach the instantiation they name (the groups above assert the same on their own launches)"""
    started = []
    for dk, insts in A16_INST.items():
        for ns, qt in insts:
            case = _length_case(dk, 33, 44)
            started.append(launch(case, 16, ns=ns, qt=qt, expect=name16(dk, ns, qt))["kernel"])
    for dk in (16, 48, 96, 128):
        for kh in (1, 2):
            case = _length_case(dk, 33, 44)
            started.append(launch(case, 32, kh=kh, expect=name32(dk, kh))["kernel"])
    print("started:", started)
    assert sorted(started) == ALL_KERNELS
