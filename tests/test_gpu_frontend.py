"""-m gpu: the STFT / log-mel front end frame by frame against float64 (tests/frontend_ref.py: cases, reference, restatements, checker).

frontend_rfft_kernel<16 | 36> (form 0, the one that runs) and frontend_kernel<16 | 36> (form 1) of csrc/htsat_frontend.hip, through
wise_debug_frontend of the debug library, which calls htsat::frontend() as both audio towers do: the grid rule, block size, template
dispatch and twiddle table are theirs.  What the two end-to-end log-mel checks never saw and these cases do:

  bins         the mel banks read FFT bins 2 .. 185 (2023) and 2 .. 325 (2022).  The tables hot0 .. hot8 read each of the 513 bins
               alone, the Nyquist line and bin 0 (the recombination's wrap to Z[0]) among them; `top` puts bands of every width up
               against bin 512, the short ones reading on through the min(start + j, 512) clamp with zero weights.
  load paths   N = 6401: clips 1 and 3 start on an odd 4-byte offset and take the reflecting scalar path on every frame, clips 0 and
               2 the 8-byte path on frames 2 .. 18; N = 6400 from an 8-byte base and from one 4 bytes on (bit-equal); N = 513, where
               the reflections at both ends meet; Fc below N / 320 + 1.
  loop trips   7 x 501 = 3507 frames, above the 3072 (rfft<16>) and 2048 (the others) frames of one trip: a ragged last workgroup
               and a ragged second trip, judged frame by frame.
  signals      white noise, un-normalised PCM (to 113 dB), DC + Nyquist, a 1000.3 Hz tone (bands at the rounding floor), silence
               (exactly -100 scale + shift), noise with a silent third; identity BatchNorm but for one case with signed scales.
Every wave buffer is [NaN | B N | NaN] and the kernel gets the interior; every table has NaN rows behind it; every output is NaN
prefilled with guard rows that must come back untouched.  A clip run alone (B = 1) is bit-equal to its rows in the batch.

Bounds: the interval and mean rules of tests/frontend_ref.py, in units of the float32 restatement's own error on the case's data.
Seen on an MI355X, per case family (over its tables) and form: R32 / M32 of the restatement; the kernel's largest
|got - dB64| / its side of the interval (1 = the bound; over the elements whose interval does not reach the 1e-10 floor) and its
largest mean |got - dB64| / mean |restated - dB64| (2 = the bound); the smallest resolved share.

  shape      tables   form   R32 max   M32 max   kernel max   kernel mean   resolved min
  n513       real     0        37.11     1.715       0.334         0.843        95.57 %
  n513       real     1        25.72     1.655       0.345         0.918        99.22 %
  n6401      real     0        14.02     1.629       0.632         0.954        99.96 %
  n6401      real     1        12.18     1.558       0.549         0.917        99.96 %
  n6400(o)   real     0        12.75     1.610       0.532         0.997        99.96 %
  n6400(o)   real     1        11.41     1.540       0.560         0.955        99.98 %
  n8000      real     0        69.66     2.056       0.350         0.800        71.56 %
  n8000      real     1        54.23     1.887       0.323         0.946        72.81 %
  n513       hot0-8   0        39.25    12.500       0.345         1.145        90.36 %
  n513       hot0-8   1        39.25    12.500       0.357         1.113        90.36 %
  n6401      hot0-8   0        68.93     9.840       0.552         1.607        88.08 %
  n6401      hot0-8   1        68.93     9.840       0.590         1.607        93.02 %
  n6400(o)   hot0-8   0        61.56     9.266       0.564         1.316        90.46 %
  n6400(o)   hot0-8   1        61.56     9.266       0.574         1.316        90.46 %
  n8000      hot0-8   0       295.01     4.881       0.364         1.068        50.00 %
  n8000      hot0-8   1       252.75     2.706       0.522         1.236        50.00 %
  n513       top      0        69.76     9.681       0.483         0.769       100.00 %
  n513       top      1        69.76     9.815       0.483         1.111       100.00 %
  n6401      top      0        89.88     7.525       0.533         1.828       100.00 %
  n6401      top      1        89.88     7.221       0.533         1.823       100.00 %
  n6400(o)   top      0        87.43     7.478       0.506         1.773       100.00 %
  n6400(o)   top      1        87.43     7.005       0.506         1.780       100.00 %
  n8000      top      0        29.15     3.324       0.137         0.590        61.25 %
  n8000      top      1        16.39     1.832       0.136         0.835        62.50 %
  big        real     0        15.34     1.894       0.613         1.409       100.00 %
  big        real     1        16.72     1.824       0.618         1.416       100.00 %
  big        hot8     0 | 1    12.37     2.356       0.594         1.176       100.00 %
  n6401r bn  real2022 0        14.02     1.839       0.546         0.990       100.00 %
  n6401r bn  real2022 1        12.17     1.757       0.564         0.993       100.00 %
(n6400o is bit-equal to n6400.)  No element comes nearer than 0.64 of the way to its bound.  The mean ratio is largest (1.8) where
PCM puts whole bands at 100 dB: there one float32 step of the result is 7.6e-6 dB, log10f on the GPU is good to about two steps
and the restatement's log10 is correctly rounded, while the transform's own share of the error is 1e-6 dB.  R32 near 300 belongs
to the single bins of the tone that hold rounding noise alone (u is its second-order term there); M32 is 12 where the only live
bin is the Nyquist line of the DC + Nyquist clip.

What these tests found when they were written: both kernels returned -100.00000763 dB, one float32 step below the floor, in every
band of a silent frame and in every band clamped at 1e-10, where float64, torch and the oracle say -100 exactly: log10f(1e-10f) on
the GPU is -10.000001 (the correctly rounded value is -10).  u is 0 on a silent frame, so the miss has no size in u; in dB it is
7.6e-6, the whole error budget of a white-noise clip, on frames that should carry none (it made the mean rule read 3.0 at the
3507-frame cases, a quarter of whose frames are silent).  Fixed in csrc/htsat_frontend.hip (power_db): the floor is the constant
-100, every value above it is computed as before.  No other fault: each of the 513 bins, both load paths, N = 513 and the second
loop trip agree with float64 within the transform's own rounding.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import audio_kernel_ref as ak
from tests import frontend_ref as fr
from wise_amd import _lib

pytestmark = pytest.mark.gpu

_P, _I = C.c_void_p, C.c_int
FORMS = (0, 1)


@functools.lru_cache(maxsize=None)
def _dbg():
    d = _lib.load_debug()
    d.wise_debug_frontend.argtypes = [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]
    d.wise_debug_frontend.restype = C.c_int
    return d


@functools.lru_cache(maxsize=None)
def _tables(table, max_band, bn):
    """the kernel's tables on the device, NaN rows behind each: hann, start, length (as floats), weights^T [36, 64], scale, shift"""
    st, ln, w = fr.table(table, max_band)
    scale, shift = fr.batchnorm(bn)
    host = dict(hann=fr.hann(), start=st.astype(np.float32), length=ln.astype(np.float32), wt=np.ascontiguousarray(w.T),
                scale=scale, shift=shift)
    return {k: ak.guarded(torch.from_numpy(v), 64).cuda() for k, v in host.items()}


def _launch(wav, offset, Fc, table, max_band, bn, form):
    """wav [B, N] float32 numpy -> what came back in the guarded output [B * Fc + GUARD, 64] (CPU)"""
    B, N = wav.shape
    buf, lead = fr.wave_buffer(wav, offset)
    dev = buf.cuda()
    assert dev.data_ptr() % 8 == 0
    t = _tables(table, max_band, bn)
    out = fr.out_buffer(B * Fc).cuda()
    d = _dbg()
    rc = d.wise_debug_frontend(dev.data_ptr() + 4 * lead, B, N, Fc, t["hann"].data_ptr(), t["start"].data_ptr(),
                               t["length"].data_ptr(), t["wt"].data_ptr(), t["scale"].data_ptr(), t["shift"].data_ptr(),
                               out.data_ptr(), max_band, form, _lib.stream_ptr())
    assert rc == 0, d.wise_last_error().decode()
    torch.cuda.synchronize()
    return out.cpu()


@functools.lru_cache(maxsize=None)
def _output(c, form):
    table, max_band, shape, bn = c
    s = fr.SHAPES[shape]
    return _launch(fr.data(shape).wav, s["offset"], s["Fc"], table, max_band, bn, form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", fr.CASES, ids=[fr.case_id(*c) for c in fr.CASES])
def test_frontend(c, form):
    full = _output(c, form)
    fr.check(fr.ref(*c), full, form)
    if c[2] == "n6400o":            # the scalar path on every frame: the same arithmetic as the 8-byte path of the aligned run
        aligned = _output((c[0], c[1], "n6400", c[3]), form)
        assert torch.equal(full.view(torch.int32), aligned.view(torch.int32)), f"{fr.case_id(*c, form)}: differs from the aligned run"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", [("real2023", 16, "n6401", 0), ("real2022", 36, "n6401", 0), ("top", 36, "n513", 0),
                               ("real2022", 36, "n6401r", 1)], ids=lambda c: fr.case_id(*c))
def test_clip_alone_equals_its_rows_in_the_batch(c, form):
    table, max_band, shape, bn = c
    s, d = fr.SHAPES[shape], fr.data(shape)
    batch = _output(c, form)
    for b in range(d.B):
        alone = _launch(d.wav[b: b + 1], (s["offset"] + b * d.N) & 1, d.Fc, table, max_band, bn, form)     # the same load path
        assert ak.guards_intact(alone, d.Fc)
        assert torch.equal(alone[: d.Fc].view(torch.int32), batch[b * d.Fc: (b + 1) * d.Fc].view(torch.int32)), \
            f"{fr.case_id(*c, form)}: clip {b} alone differs from the batch"


def test_form_is_the_twins_argument():
    """the twin runs the form it is asked for whatever the towers' own switch (wise_debug_set_htsat bit 5) says, and the two
    forms are different kernels: their outputs differ in the last bits"""
    d = _dbg()
    c = ("real2023", 16, "n6400", 0)
    want = [_output(c, form) for form in FORMS]
    assert not torch.equal(want[0].view(torch.int32), want[1].view(torch.int32))
    d.wise_debug_set_htsat.argtypes, d.wise_debug_set_htsat.restype = [_I], C.c_int
    try:
        d.wise_debug_set_htsat(1 << 5)
        got = [_launch(fr.data("n6400").wav, 0, 21, "real2023", 16, 0, form) for form in FORMS]
    finally:
        d.wise_debug_set_htsat(0)
    for form in FORMS:
        assert torch.equal(got[form].view(torch.int32), want[form].view(torch.int32))


def test_debug_entry_refuses_other_shapes():
    d, st = _dbg(), _lib.stream_ptr()
    p = torch.zeros(1 << 16, device="cuda").data_ptr()      # large enough for every shape below but the last, were one let through

    def refused(rc):
        assert rc != 0 and b"debug_frontend" in d.wise_last_error(), (rc, d.wise_last_error())

    for B, N, Fc, mb, form in ((0, 6400, 21, 16, 0), (1, 512, 1, 16, 0), (1, 6400, 0, 16, 0), (1, 6400, 22, 16, 0),
                               (1, 6401, 21, 0, 0), (1, 6401, 21, 37, 0), (1, 6401, 21, 16, 2), (1, 6401, 21, 16, -1),
                               (33555, 320000, 1001, 16, 0)):
        refused(d.wise_debug_frontend(p, B, N, Fc, p, p, p, p, p, p, p, mb, form, st))
    for hole in range(8):
        args = [p] * 8
        args[hole] = 0
        refused(d.wise_debug_frontend(args[0], 1, 6400, 21, *args[1:], 16, 0, st))
    refused(d.wise_debug_frontend(p + 2, 1, 6400, 21, p, p, p, p, p, p, p, 16, 0, st))
