"""The order in which a run entry reports the faults of a call (include/vitsmi.h), without a GPU: every whole-path entry and
every chunked vocoder entry, by name, on a host-only handle, with calls that carry two faults at once - which of them
vits_last_error holds afterwards is the order.  One order serves all entries, each taking the steps it has arguments for:
null handle, stream format, stream shaping, stream onsets, fit, intonation (with its null controls), the device, the
controls (forced durations among them)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

PATH = os.path.join(GOLDEN, "tiny_rb1.onnx")
B, T, F = 2, 5, 6
E_ARG, E_DEVICE = -3, -4

# entry -> (settings: "one" [3] scales / "rows" / "ctl" / None for the vocoder, extra: "fit" / "warp" / "glide" / None,
#           sink: "async" / "out" / "f32" / "enc" / "shaped" / "trimmed")
ENTRIES = {
    "vits_run": ("one", None, "out"),
    "vits_run_async": ("one", None, "async"),
    "vits_run_async_rows": ("rows", None, "async"),
    "vits_run_async_ctl": ("ctl", None, "async"),
    "vits_run_async_fitted": ("ctl", "fit", "async"),
    "vits_run_async_warped": ("ctl", "warp", "async"),
    "vits_run_async_glided": ("ctl", "glide", "async"),
    "vits_run_chunked": ("one", None, "f32"),
    "vits_run_chunked_rows": ("rows", None, "f32"),
    "vits_run_chunked_ctl": ("ctl", None, "f32"),
    "vits_run_chunked_fitted": ("ctl", "fit", "f32"),
    "vits_run_chunked_glided": ("ctl", "glide", "f32"),
    "vits_run_chunked_enc": ("ctl", None, "enc"),
    "vits_run_chunked_enc_shaped": ("ctl", None, "shaped"),
    "vits_run_chunked_enc_trimmed": ("ctl", None, "trimmed"),
    "vits_run_chunked_enc_fitted": ("ctl", "fit", "trimmed"),
    "vits_run_chunked_enc_glided": ("ctl", "glide", "trimmed"),
    "vits_run_vocoder_chunked": (None, None, "f32"),
    "vits_run_vocoder_chunked_enc": (None, None, "enc"),
    "vits_run_vocoder_chunked_enc_shaped": (None, None, "shaped"),
    "vits_run_vocoder_chunked_enc_trimmed": (None, None, "trimmed"),
}
# the entries whose controls are looked at (by the intonation's checks) before the device is
INTONED = [n for n, (_, extra, _) in ENTRIES.items() if extra in ("warp", "glide")]

UNKNOWN_ENCODING, BAD_SHAPING, BAD_ONSETS = "unknown encoding 9", "lookahead -1 outside", "row 0: onset mode 7 outside 0..2"
BAD_FIT, BAD_SEMITONE, HOST_ONLY = "fit mode[0]=5", "[0,1]=40 is not a finite value within [-12, 12]", "host-only"


def entries(settings=None, extra=None, sink=None):
    """the names of the entries that take the arguments concerned"""
    return [n for n, (s, e, k) in ENTRIES.items()
            if (settings is None or s in settings) and (extra is None or e in extra) and (sink is None or k in sink)]


@pytest.fixture(scope="module")
def host():
    from phoonnx_amd import MiSession
    s = MiSession(PATH, host_only=True)
    yield s
    s.close()


def call(s, name, null_handle=False, encoding=0, bad_shaping=False, bad_onsets=False, bad_fit=False, bad_semitone=False,
         negative_duration=False, null_ctl=False, bad_rows=False):
    """one call of entry `name` with the faults asked for and everything else in order -> (rc, vits_last_error)"""
    from phoonnx_amd import _ffi
    settings, extra, sink = ENTRIES[name]
    h = None if null_handle else s._h
    ids, lens = np.ones((B, T), np.int64), np.array([T, 3], np.int64)
    scales = np.array([0.667, 1.0, 0.8], np.float32)
    rows = np.tile(scales, (B, 1))
    rows[0, 0] = np.nan if bad_rows else rows[0, 0]
    noise = _ffi.VitsNoise()
    durations = np.full((B, T), 2, np.int64)
    durations[0, 1] = -4
    ctl = _ffi.VitsControls(rows.ctypes.data, None, durations.ctypes.data if negative_duration else None, None)
    ctl = None if null_ctl else C.byref(ctl)
    if settings is None:
        z = np.zeros((B, s.hparam("inter"), F), np.float32)
        args = [h, _ffi.ptr(z), B, F, None]
    elif settings == "one":
        args = [h, _ffi.ptr(ids), _ffi.ptr(lens), B, T, _ffi.ptr(scales), None, C.byref(noise)]
    elif settings == "rows":
        args = [h, _ffi.ptr(ids), _ffi.ptr(lens), B, T, _ffi.ptr(rows), None, C.byref(noise), None]
    else:
        args = [h, _ffi.ptr(ids), _ffi.ptr(lens), B, T, None, C.byref(noise), ctl]
    fmt = _ffi.VitsStreamFormat(encoding, None, None)
    shaping = _ffi.VitsStreamShaping()
    shaping.lookahead = -1 if bad_shaping else 0
    onsets = (_ffi.VitsStreamOnset * B)()
    onsets[0].mode = 7 if bad_onsets else 0
    if sink in ("enc", "shaped", "trimmed"):
        args.append(C.byref(fmt))
    if sink in ("shaped", "trimmed"):
        args.append(C.byref(shaping))
    if sink == "trimmed":
        args.append(onsets)
    group, target, mode = np.zeros(B, np.int32), np.array([9], np.int64), np.array([5 if bad_fit else 1], np.int32)
    st = np.zeros((B, T), np.float32)
    st[0, 1] = 40.0 if bad_semitone else 2.0
    if extra == "fit":
        fit = _ffi.VitsFit(group.ctypes.data, 1, target.ctypes.data, mode.ctypes.data)
        args.append(C.byref(fit))
    elif extra == "warp":
        into = _ffi.VitsIntonation(st.ctypes.data, 0)
        args.append(C.byref(into))
    elif extra == "glide":
        contour = _ffi.VitsContour(st.ctypes.data, None, 0)
        args.append(C.byref(contour))
    out = _ffi.VitsOutput()
    if sink == "out":
        args.append(C.byref(out))
    elif sink != "async":
        fn = {"f32": _ffi.CHUNK_FN, "trimmed": _ffi.ENC_CHUNK_TRIM_FN}.get(sink, _ffi.ENC_CHUNK_FN)(lambda *a: 0)
        args += [8, fn, None]
    rc = getattr(s._lib, name)(*args)
    return rc, s._err()


def test_every_run_entry_is_listed():
    from phoonnx_amd import _ffi
    runs = {n for n in _ffi.EXPORTS if n.startswith(("vits_run_async", "vits_run_chunked", "vits_run_vocoder_chunked"))} | {"vits_run"}
    assert runs == set(ENTRIES)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_a_faultless_call_gets_as_far_as_the_device(host, name):
    assert call(host, name) == (E_DEVICE, "handle was opened host-only")


@pytest.mark.parametrize("name", list(ENTRIES))
def test_a_null_handle_is_refused_first(host, name):
    """... whatever else is wrong with the call, and without a message on any handle"""
    _, extra, sink = ENTRIES[name]
    call(host, name)
    faults = dict(encoding=9 if sink in ("enc", "shaped", "trimmed") else 0, bad_shaping=True, bad_onsets=True, bad_fit=True,
                  bad_semitone=True, negative_duration=True)
    assert call(host, name, null_handle=True, **faults) == (E_ARG, "handle was opened host-only")
    assert call(host, name, null_handle=True, null_ctl=True)[0] == E_ARG


@pytest.mark.parametrize("name", entries(extra=("fit",), sink=("trimmed",)))
def test_the_format_is_answered_before_the_fit(host, name):
    rc, err = call(host, name, encoding=9, bad_fit=True)
    assert rc == E_ARG and err == UNKNOWN_ENCODING


@pytest.mark.parametrize("name", entries(sink=("trimmed",)))
def test_the_shaping_is_answered_before_the_onsets(host, name):
    rc, err = call(host, name, bad_shaping=True, bad_onsets=True)
    assert rc == E_ARG and BAD_SHAPING in err and "onset" not in err, err
    rc, err = call(host, name, encoding=9, bad_shaping=True, bad_onsets=True)     # ... and the format before both
    assert rc == E_ARG and err == UNKNOWN_ENCODING


@pytest.mark.parametrize("name", entries(extra=("fit",), sink=("trimmed",)))
def test_the_onsets_are_answered_before_the_fit(host, name):
    rc, err = call(host, name, bad_onsets=True, bad_fit=True)
    assert rc == E_ARG and err == BAD_ONSETS


@pytest.mark.parametrize("name", entries(extra=("glide",), sink=("trimmed",)))
def test_the_onsets_are_answered_before_the_intonation(host, name):
    rc, err = call(host, name, bad_onsets=True, bad_semitone=True)
    assert rc == E_ARG and err == BAD_ONSETS


@pytest.mark.parametrize("name", entries(extra=("fit",)))
def test_a_bad_fit_is_answered_before_the_device(host, name):
    rc, err = call(host, name, bad_fit=True)
    assert rc == E_ARG and BAD_FIT in err and HOST_ONLY not in err, err


@pytest.mark.parametrize("name", INTONED)
def test_a_semitone_out_of_range_is_answered_before_the_device(host, name):
    rc, err = call(host, name, bad_semitone=True)
    assert rc == E_ARG and err == "token_semitones" + BAD_SEMITONE


@pytest.mark.parametrize("name", entries(settings=("ctl",)))
def test_a_negative_forced_duration_is_answered_behind_the_device(host, name):
    """the controls' own values are checked last, by every entry: the host-only handle is what the call reports - unless a
    fit, which is answered before the device, refuses forced durations as such"""
    want = (E_DEVICE, "handle was opened host-only")
    if ENTRIES[name][1] == "fit":
        want = (E_ARG, "durations and a fit are contradictory: forced durations leave nothing to fit")
    assert call(host, name, negative_duration=True) == want


@pytest.mark.parametrize("name", entries(settings=("ctl",)))
def test_null_controls_are_answered_by_the_intonation_or_behind_the_device(host, name):
    """the intonation reads the controls, so its entries refuse a null pointer on the host; the others look at the device first"""
    want = (E_ARG, "null argument") if name in INTONED else (E_DEVICE, "handle was opened host-only")
    assert call(host, name, null_ctl=True) == want
    if ENTRIES[name][1] == "fit":  # (the fit's own values do not need the controls)
        rc, err = call(host, name, null_ctl=True, bad_fit=True)
        assert rc == E_ARG and BAD_FIT in err, err


@pytest.mark.parametrize("name", entries(settings=("rows",)))
def test_a_row_that_is_not_finite_is_answered_behind_the_device(host, name):
    assert call(host, name, bad_rows=True) == (E_DEVICE, "handle was opened host-only")


@pytest.mark.parametrize("name", entries(extra=("glide",), sink=("trimmed",)))
def test_null_controls_of_an_intoned_stream_are_answered_behind_the_stream_checks(host, name):
    rc, err = call(host, name, null_ctl=True, bad_onsets=True)
    assert rc == E_ARG and err == BAD_ONSETS
