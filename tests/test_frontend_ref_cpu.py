"""No GPU: tests/frontend_ref.py held to account.  The float64 reference agrees with torch's reflect padding and stft and the
oracle's filterbank; the float32 restatement of each form passes the checker on every case and stays within R32_MAX units of float64; the
clips that must be resolved are; the hot tables read every bin once; and the checker fails each planted fault, applied to an
otherwise exact output (which itself passes)."""
import numpy as np
import pytest
import torch

from oracle import htsat_ref
from tests import frontend_ref as fr

FORMS = (0, 1)


@pytest.mark.parametrize("c", fr.CASES, ids=[fr.case_id(*c) for c in fr.CASES])
def test_restatements_pass_and_resolve(c):
    r = fr.ref(*c)
    for form in FORMS:
        fig = fr.check(r, fr.as_output(r.db32[form]), form)
        assert fig["max ratio"] <= 0.75       # |P32 - P64| <= R32 u = T / 4; the rest is the log's slope and d
        shares = r.resolved_by_clip(form)
        print(f"{fig['what']}: resolved share per clip " + ", ".join(f"{k} {s:.4f}" for k, s in shares))
        for kind, share in shares:
            if kind in ("noise", "pcm") or fr.all_resolved(c[2]):
                assert share == 1.0, f"{fig['what']}: {100 * share:.3f} % of a {kind} clip is resolved"
        fr.check(r, fr.as_output(r.db64), form)          # and so does the float64 value itself, rounded once


def test_case_table():
    ids = [fr.case_id(*c) for c in fr.CASES]
    assert len(set(ids)) == len(ids)
    bins = np.concatenate([fr.table(f"hot{t}", 16)[0][: (1 if t == 8 else 64)] for t in range(9)])
    assert sorted(bins.tolist()) == list(range(fr.BINS))                  # the nine hot tables read every bin alone
    for mb in (16, 36):
        st, ln, w = fr.table("top", mb)
        assert set(ln.tolist()) == set(range(1, mb + 1)) and bool((st + ln == fr.BINS).all()) and bool((w[:, 0] > 0).all())
    assert int(fr.table("real2023", 16)[1].max()) == 16 and int(fr.table("real2022", 36)[1].max()) == 35
    s = fr.SHAPES["big"]
    assert s["B"] * s["Fc"] == 3507 > 3072 and (3507 - 3072) % 4 != 0 and (3507 - 2048) % 4 != 0   # ragged second trip
    for name, s in fr.SHAPES.items():
        assert s["N"] >= 513 and 1 <= s["Fc"] <= s["N"] // 320 + 1
    assert all(fr.all_resolved(s) for s in ("big", "n6401r")) and not any(fr.all_resolved(s) for s in fr.SMALL)
    # which frames of n6401 / n6400 lie inside their clip (the 8-byte load, where the address allows it)
    inside = [f for f in range(21) if f * 320 - 512 >= 0 and f * 320 + 512 <= 6400]
    assert inside == list(range(2, 19))
    buf, lead = fr.wave_buffer(fr.data("n6400").wav, 1)
    assert lead % 2 == 1 and bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + 4 * 6400:]).all())


@pytest.mark.parametrize("shape", ("n513", "n6401"))
def test_float64_reference_against_the_oracle(shape):
    d = fr.data(shape)
    wav = torch.from_numpy(d.wav).double()
    x = torch.nn.functional.pad(wav[:, None], (512, 512), mode="reflect")[:, 0]               # reflect and transform by torch
    S = torch.stft(x, 1024, 320, window=htsat_ref.hann_periodic().double(), center=False, return_complex=True)
    want = (S.abs() ** 2).permute(0, 2, 1)[:, : d.Fc].reshape(d.rows, fr.BINS).numpy()
    scale = want.max(axis=1, keepdims=True)
    assert np.abs(d.P64 - want).max() <= 1e-6 * scale.max() and (np.abs(d.P64 - want) <= 1e-6 * scale + 1e-30).all()
    r = fr.ref("real2023", 16, shape, 0)
    mel = want @ htsat_ref.mel_filterbank().astype(np.float64).T
    np.testing.assert_allclose(r.P64, mel, rtol=1e-5, atol=1e-9 * mel.max())


# ------------------------------------------------------------------------------------------------ planted faults
def _exact(r, frames_kw=None, window=None, mutate=None, scale=None):
    """the float64 pipeline of case `r`, with a fault planted, as the output buffer a kernel would leave"""
    d = r.d
    frames = fr.frames_of(d.wav, d.Fc, **(frames_kw or {}))
    X, _ = fr.spectrum64(frames, d.window if window is None else window)
    P = X.real ** 2 + X.imag ** 2
    if mutate:
        P = mutate(P, frames.astype(np.float64) * d.window.astype(np.float64))
    return fr.as_output(fr.db64(P @ fr.dense(r.st, r.ln, r.w).T, r.scale if scale is None else scale, r.shift))


def _swap(P, x):
    P = P.copy()
    P[:, [300, 301]] = P[:, [301, 300]]
    return P


def _nyquist_is_511(P, x):
    P = P.copy()
    P[:, 512] = P[:, 511]
    return P


def _bin0_without_O(P, x):
    P = P.copy()
    P[:, 0] = x[:, 0::2].sum(axis=1) ** 2          # X[0] = E[0] - i O[0] = Re Z[0] + Im Z[0]; E[0] alone is the even samples' sum
    return P


def _second_trip(full):
    full = full.clone()
    full[3100] = full[3100 - 3072]
    return full


def _past_the_end(full, rows):
    full = full.clone()
    full[rows] = full[rows - 1]
    return full


_symmetric_hann = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1024) / 1023)).astype(np.float32)

FAULTS = {
    # name: (case, how the exact output is spoilt)
    "adjacent bins swapped": (("hot4", 16, "n6401", 0), lambda r: _exact(r, mutate=_swap)),
    "bin 512 taken as bin 511": (("hot8", 36, "n6401", 0), lambda r: _exact(r, mutate=_nyquist_is_511)),
    "bin 0 without the O term": (("hot0", 16, "n6401", 0), lambda r: _exact(r, mutate=_bin0_without_O)),
    "frame start off by one": (("real2023", 16, "n6401", 0), lambda r: _exact(r, dict(shift=1))),
    "zero padding at the clip end": (("real2023", 16, "n6401", 0), lambda r: _exact(r, dict(zero_pad_end=True))),
    "symmetric Hann": (("real2023", 16, "n6400", 0), lambda r: _exact(r, window=_symmetric_hann)),
    "clip stride N - 1": (("real2022", 36, "n6401", 0), lambda r: _exact(r, dict(stride=r.d.N - 1))),
    "second trip repeats the first": (("real2023", 16, "big", 0), lambda r: _second_trip(_exact(r))),
    "BatchNorm scale of lane m ^ 1": (("real2022", 36, "n6401r", 1), lambda r: _exact(r, scale=r.scale[np.arange(64) ^ 1])),
    "a row past the end": (("real2023", 16, "n513", 0), lambda r: _past_the_end(_exact(r), r.rows)),
}


@pytest.mark.parametrize("name", list(FAULTS))
def test_checker_fails_planted_fault(name):
    c, spoil = FAULTS[name]
    r = fr.ref(*c)
    good, bad = _exact(r), spoil(r)
    assert not torch.equal(good.view(torch.int32), bad.view(torch.int32))
    for form in FORMS:
        fr.check(r, good, form)
        with pytest.raises(AssertionError, match="guard rows" if name == "a row past the end" else "outside the interval"):
            fr.check(r, bad, form)


@pytest.mark.parametrize("form", FORMS)
def test_mean_rule_catches_a_coarse_twiddle_table(form):
    """a twiddle table with 1e-5 relative error: the mean rule alone must refuse it"""
    r = fr.ref("real2023", 16, "big", 0)
    d = r.d
    P = fr.power32(fr.frames_of(d.wav, d.Fc), d.window, form, fr.twiddles(rel_err=1e-5))
    fig = fr.measure(r, fr.as_output(fr.db32(fr.band32(P, r.st, r.ln, r.w), r.scale, r.shift)), form)
    print(f"{fig['what']}: mean ratio {fig['mean ratio']:.2f}, {int(fig['outside'].sum())} elements outside the interval")
    assert fig["mean ratio"] > 2
    with pytest.raises(AssertionError):
        fr.check(r, fr.as_output(fr.db32(fr.band32(P, r.st, r.ln, r.w), r.scale, r.shift)), form)
