"""The STFT / log-mel front end (csrc/htsat_frontend.hip) frame by frame: the case table, a float64 reference, a float32
restatement of each of the kernel's two transforms, and the checker.  Plain numpy on the CPU: tests/test_gpu_frontend.py runs
the kernels against it through wise_debug_frontend, tests/test_frontend_ref_cpu.py holds the restatements and the checker
(against planted faults) to account without a GPU.  Guard helpers and NaN patterns are those of tests/audio_kernel_ref.py.

  float64     frames by the reflect rule s = |320 f - 512 + n|, 2 (N - 1) - s where s >= N; times the fp32 Hann table;
              numpy.fft.rfft; power; the dense [64, 513] band matrix of the sparse table the kernel is handed;
              10 log10(max(P, 1e-10)) * scale + shift
  float32     form 1: the 1024-point radix-2 decimation-in-time transform, butterflies in the textbook order; form 0: the
              512-point transform of z[n] = x[2n] + i x[2n+1] and the kernel's recombination.  Twiddles rounded from float64, no
              fma anywhere, the band sum a sequential chain, log10 rounded once to float32.  This is the measuring stick: it says what fp32
              arithmetic costs on the data of a case, and every bound is a multiple of ITS error, never of the kernel's.

The rounding unit of element (frame, band m): u = e sum_j w_mj (|X_j| A + e A^2), with X the float64 spectrum of the frame,
A = ||frame * hann||_2, e = 2^-24: the first-order size of an fp32 FFT's error in that band's power.  Per case and form
R32 = max and M32 = mean of |P32 - P64| / u over the elements with u > 0 (P32: the restatement's band power before its log).

  interval    every element: with T = 4 R32 u the kernel's value lies in [dB(max(P64 - T, 1e-10)) - d, dB(max(P64 + T, 1e-10)) + d],
              d = 4 e max(|dB64|, 1) for log10f, the multiply by 10 and the BatchNorm fma (dB before BatchNorm, d times |scale|).
              4 is the margin over a maximum taken over 1e3 .. 2e5 elements of the same statistics; what this is to catch (a wrong
              bin, sample or twiddle, stale LDS, a dropped Nyquist line) is beyond 1e4 u.
  mean        over the resolved elements (T <= 1e-2 max(P64, 1e-10)): mean |got - dB64| <= 2 mean |restated - dB64|: systematic
              precision loss that stays inside the interval, such as a twiddle table from a less accurate sincos.
  exact       a frame of zeros gives -100 scale + shift exactly, in every band: float32's value of it, whether from one fma or
              from a rounded product and a sum (the two differ only where scale is not 1).
  R32 itself  at most R32_MAX = 1024.  Where a bin carries signal the restatements sit at 10 .. 90 u; in the bins of a tone that
              hold rounding noise alone u is its second-order term e^2 A^2 and the error (c e A)^2 with c up to 17, so R32 reaches
              300.  At 1024 the interval is 4096 u, still under the smallest fault above; a restatement that is wrong sits at 1e6
              and would excuse anything.
"""
import functools

import numpy as np
import torch

from tests.audio_kernel_ref import GUARD, guards_intact, nan_rows
from wise_amd.feature import htsat_frontend as fe

E = 2.0 ** -24
N_FFT, HOP, BANDS, BINS, MELW = 1024, 320, 64, 513, fe.MELW
WAVE_GUARD = 1024            # floats of NaN on either side of a wave buffer (even: keeps the interior's 8-byte phase)
R32_MAX = 1024.0
FLOOR = 1e-10

# ------------------------------------------------------------------------------------------------ the case table
# kinds: one signal per clip.  Resolved everywhere (asserted): noise, pcm, gap, zeros; dcnyq and tone leave bands at the rounding floor.
SHAPES = {
    "n513": dict(B=3, N=513, Fc=2, kinds=("noise", "tone", "dcnyq"), offset=0),       # the smallest clip; reflection at both ends meets
    "n6401": dict(B=4, N=6401, Fc=21, kinds=("noise", "pcm", "gap", "dcnyq"), offset=0),   # clips 1, 3 on an odd 4-byte offset
    "n6400": dict(B=4, N=6400, Fc=21, kinds=("noise", "pcm", "gap", "dcnyq"), offset=0),   # 8-byte path on frames 2 .. 18
    "n6400o": dict(B=4, N=6400, Fc=21, kinds=("noise", "pcm", "gap", "dcnyq"), offset=1),  # the same from a base 4 bytes on
    "n6401r": dict(B=4, N=6401, Fc=21, kinds=("noise", "pcm", "gap", "zeros"), offset=0),   # the BatchNorm case: all resolved
    "n8000": dict(B=2, N=8000, Fc=10, kinds=("tone", "zeros"), offset=0),             # fewer frames than the clip holds
    # 3507 frames: above both grid caps (3072 and 2048 frames a trip), ragged last workgroup, ragged second trip
    "big": dict(B=7, N=160000, Fc=501, kinds=("noise", "pcm", "gap", "zeros", "pcm", "noise", "gap"), offset=0),
}
SMALL = ("n513", "n6401", "n6400", "n6400o", "n8000")
TABLES = [("real2023", 16), ("real2022", 36)] + [(f"hot{t}", mb) for t in range(9) for mb in (16, 36)] + [("top", 16), ("top", 36)]
BIG_TABLES = [("real2023", 16), ("real2022", 36), ("hot8", 16)]
# (table, max_band, shape, bn): every table at every small shape, three at the large one, and the one BatchNorm case
CASES = ([(t, mb, s, 0) for t, mb in TABLES for s in SMALL] + [(t, mb, "big", 0) for t, mb in BIG_TABLES]
         + [("real2022", 36, "n6401r", 1)])
RESOLVED_KINDS = ("noise", "pcm", "gap", "zeros")


def case_id(table, max_band, shape, bn, form=None):
    return f"{table}-mb{max_band}-{shape}" + ("-bn" if bn else "") + ("" if form is None else f"-form{form}")


def all_resolved(shape):
    """the cases whose every element must be resolved (the 3507 frames, the BatchNorm case): clips of RESOLVED_KINDS only"""
    return all(k in RESOLVED_KINDS for k in SHAPES[shape]["kinds"])


# ------------------------------------------------------------------------------------------------ signals and tables
def signal(kind, N, rng):
    n = np.arange(N)
    if kind == "noise":
        x = 0.1 * rng.standard_normal(N)
    elif kind == "pcm":                                  # un-normalised 16-bit samples: dB up to about 113
        x = np.rint(8000 * rng.standard_normal(N))
    elif kind == "dcnyq":                                # DC and Nyquist carry almost everything
        x = 0.25 + 0.5 * (1 - 2 * (n & 1)) + 1e-3 * rng.standard_normal(N)
    elif kind == "tone":                                 # most bands are rounding floor or clamp
        x = 0.5 * np.sin(2 * np.pi * 1000.3 * n / fe.SR)
    elif kind == "zeros":
        x = np.zeros(N)
    else:
        assert kind == "gap"                             # frames partly and wholly silent inside a live clip
        x = 0.1 * rng.standard_normal(N)
        x[N // 3: 2 * N // 3] = 0
    return x.astype(np.float32)


def waves(B, N, Fc, kinds):
    """[B, N] float32, seeded by the data alone: n6400 and n6400o are the same samples"""
    rng = np.random.default_rng([B, N, Fc])
    return np.stack([signal(k, N, rng) for k in kinds])


def table(name, max_band):
    """(start [64] int, length [64] int, weights [64, MELW] float32), the sparse form the kernel is handed"""
    if name in ("real2023", "real2022"):
        st, ln, w = fe.sparse_mel(8000.0 if name == "real2023" else 14000.0)
        st, ln, w = st.numpy().astype(np.int64), ln.numpy().astype(np.int64), w.numpy()
    elif name.startswith("hot"):                         # band m is one bin alone: hot0 .. hot8 read every one of the 513
        t = int(name[3:])
        st = np.full(BANDS, 512, np.int64) if t == 8 else 64 * t + np.arange(BANDS)
        ln, w = np.ones(BANDS, np.int64), np.zeros((BANDS, MELW), np.float32)
        w[:, 0] = 1
    else:
        assert name == "top"                             # bands of every width that end exactly at the Nyquist bin
        rng = np.random.default_rng(max_band)
        ln = 1 + np.arange(BANDS) % max_band
        st = BINS - ln
        w = np.where(np.arange(MELW)[None] < ln[:, None], rng.uniform(0.005, 0.05, (BANDS, MELW)), 0).astype(np.float32)
    assert int(ln.max()) <= max_band <= MELW and int((st + ln).max()) <= BINS
    return st, ln, w


def dense(st, ln, w):
    """[64, 513] float64"""
    W = np.zeros((BANDS, BINS))
    for m in range(BANDS):
        W[m, st[m]: st[m] + ln[m]] = w[m, : ln[m]]
    return W


def batchnorm(bn):
    """(scale [64], shift [64]) float32: identity, or |scale| in 0.5 .. 2 with every third sign negative and |shift| <= 0.5"""
    if not bn:
        return np.ones(BANDS, np.float32), np.zeros(BANDS, np.float32)
    rng = np.random.default_rng(1234)
    scale = rng.uniform(0.5, 2.0, BANDS) * np.where(np.arange(BANDS) % 3 == 1, -1, 1)
    return scale.astype(np.float32), rng.uniform(-0.5, 0.5, BANDS).astype(np.float32)


def hann():
    return fe.hann_periodic().numpy()


# ------------------------------------------------------------------------------------------------ float64
def frame_index(N, Fc, shift=0):
    """[Fc, 1024] sample index of every tap by the reflect rule (`shift`: a planted off-by-one)"""
    s = np.abs(np.arange(Fc)[:, None] * HOP - N_FFT // 2 + np.arange(N_FFT)[None] + shift)
    return np.where(s >= N, 2 * (N - 1) - s, s)


def frames_of(wav, Fc, shift=0, zero_pad_end=False, stride=None):
    """[B * Fc, 1024] in the dtype of `wav` [B, N]; the keywords plant faults"""
    B, N = wav.shape
    idx = frame_index(N, Fc, shift)
    flat = wav.reshape(-1)
    out = []
    for b in range(B):
        base = b * N if stride is None or b != 1 else stride
        fr = flat[base + idx]
        if zero_pad_end:
            raw = np.arange(Fc)[:, None] * HOP - N_FFT // 2 + np.arange(N_FFT)[None]
            fr = np.where(raw >= N, 0, fr)
        out.append(fr)
    return np.concatenate(out)


def spectrum64(frames, window):
    """-> (X [F, 513] complex128, A [F])"""
    x = frames.astype(np.float64) * window.astype(np.float64)
    return np.fft.rfft(x, axis=1), np.sqrt((x * x).sum(axis=1))


def db64(P, scale, shift):
    return 10 * np.log10(np.maximum(P, FLOOR)) * scale.astype(np.float64) + shift.astype(np.float64)


# ------------------------------------------------------------------------------------------------ float32
def twiddles(rel_err=0.0):
    """(re, im) [1024] float32: tw[half + j] = exp(-i pi j / half), rounded from float64 (`rel_err`: a planted fault)"""
    re, im = np.ones(1024), np.zeros(1024)
    half = 1
    while half < 1024:
        x = np.arange(half) / half
        c, s = np.cos(np.pi * x), np.sin(np.pi * x)
        c[x == 0.5] = 0
        re[half: 2 * half], im[half: 2 * half] = c, -s
        half *= 2
    if rel_err:
        rng = np.random.default_rng(5)
        re, im = re * (1 + rel_err * rng.standard_normal(1024)), im * (1 + rel_err * rng.standard_normal(1024))
    return re.astype(np.float32), im.astype(np.float32)


def bit_reverse(n):
    bits = n.bit_length() - 1
    i = np.arange(n)
    r = np.zeros(n, np.int64)
    for b in range(bits):
        r |= ((i >> b) & 1) << (bits - 1 - b)
    return r


def dit32(re, im, tw):
    """radix-2 decimation in time on [F, n] float32 (natural order in, natural order out), stage by stage"""
    twr, twi = tw
    F, n = re.shape
    rev = bit_reverse(n)
    re, im = re[:, rev], im[:, rev]
    half = 1
    while half < n:
        r, i = re.reshape(F, n // (2 * half), 2, half), im.reshape(F, n // (2 * half), 2, half)
        ar, ai, qr, qi = r[:, :, 0], i[:, :, 0], r[:, :, 1], i[:, :, 1]
        cr, ci = twr[half: 2 * half], twi[half: 2 * half]
        tr, ti = cr * qr - ci * qi, cr * qi + ci * qr
        re = np.stack([ar + tr, ar - tr], axis=2).reshape(F, n)
        im = np.stack([ai + ti, ai - ti], axis=2).reshape(F, n)
        half *= 2
    assert re.dtype == np.float32 and im.dtype == np.float32
    return re, im


def power32(frames, window, form, tw=None):
    """[F, 1024] float32 frames -> [F, 513] float32 power, as the kernel's form computes it"""
    tw = tw or twiddles()
    x = frames.astype(np.float32) * window.astype(np.float32)
    if form == 1:
        re, im = dit32(x, np.zeros_like(x), tw)
        return (re * re + im * im)[:, :BINS]
    zr, zi = dit32(np.ascontiguousarray(x[:, 0::2]), np.ascontiguousarray(x[:, 1::2]), tw)
    k = np.arange(512)
    cr, ci = zr[:, (512 - k) & 511], zi[:, (512 - k) & 511]
    h = np.float32(0.5)
    ex, ey, ox, oy = h * (zr + cr), h * (zi - ci), h * (zr - cr), h * (zi + ci)
    wr, wi = tw[0][512:], tw[1][512:]
    xr, xi = ex + (wr * oy + wi * ox), ey - (wr * ox - wi * oy)
    ny = zr[:, :1] - zi[:, :1]
    P = np.concatenate([xr * xr + xi * xi, ny * ny], axis=1)
    assert P.dtype == np.float32
    return P


def band32(P, st, ln, w):
    """[F, 513] float32 -> [F, 64] float32: acc = acc + w_j P[min(start + j, 512)], j ascending, no fma"""
    acc = np.zeros((P.shape[0], BANDS), np.float32)
    for j in range(int(ln.max())):
        wj = np.where(j < ln, w[:, j], 0).astype(np.float32)
        acc = acc + wj[None] * P[:, np.minimum(st + j, 512)]
    return acc


def db32(acc, scale, shift):
    # log10 correctly rounded to float32 (numpy's own float32 log10 is a few steps off, -10 at the floor included)
    db = np.float32(10) * np.log10(np.maximum(acc, np.float32(FLOOR)).astype(np.float64)).astype(np.float32)
    out = db * scale[None] + shift[None]
    assert out.dtype == np.float32
    return out


# ------------------------------------------------------------------------------------------------ references, built once
class Data:
    """one data set (shape without its base offset): waves, float64 spectrum, the two float32 power spectra"""

    def __init__(self, B, N, Fc, kinds):
        self.B, self.N, self.Fc, self.kinds = B, N, Fc, kinds
        self.wav = waves(B, N, Fc, kinds)
        self.window = hann()
        fr = frames_of(self.wav, self.Fc)
        self.X, self.A = spectrum64(fr, self.window)
        self.P64 = self.X.real ** 2 + self.X.imag ** 2
        self.unit = E * (np.abs(self.X) * self.A[:, None] + E * (self.A ** 2)[:, None])      # per bin: u = unit @ W^T
        self.P32 = {form: power32(fr, self.window, form) for form in (0, 1)}
        self.silent = ~fr.any(axis=1)
        self.rows = self.B * self.Fc


@functools.lru_cache(maxsize=None)
def _data(B, N, Fc, kinds):
    return Data(B, N, Fc, kinds)


def data(shape):
    s = SHAPES[shape]
    return _data(s["B"], s["N"], s["Fc"], s["kinds"])            # n6400o is n6400's data


class Ref:
    """one case: table + BatchNorm on a data set; per form the restatement's band power, dB and its R32, M32"""

    def __init__(self, table_name, max_band, shape, bn):
        self.what = case_id(table_name, max_band, shape, bn)
        self.shape, self.max_band, self.bn = shape, max_band, bn
        self.d = d = data(shape)
        self.st, self.ln, self.w = table(table_name, max_band)
        self.scale, self.shift = batchnorm(bn)
        W = dense(self.st, self.ln, self.w)
        self.P64 = d.P64 @ W.T
        self.u = d.unit @ W.T
        self.db64 = db64(self.P64, self.scale, self.shift)
        # -100 scale + shift in float32: as one fma, or as a rounded product and a sum (they differ only under BatchNorm)
        self.silent_value = ((-100.0 * self.scale.astype(np.float64) + self.shift.astype(np.float64)).astype(np.float32),
                             np.float32(-100) * self.scale + self.shift)
        self.P32, self.db32, self.R32, self.M32 = {}, {}, {}, {}
        live = self.u > 0
        for form in (0, 1):
            acc = band32(d.P32[form], self.st, self.ln, self.w)
            self.P32[form], self.db32[form] = acc, db32(acc, self.scale, self.shift)
            ratio = np.abs(acc.astype(np.float64) - self.P64)[live] / self.u[live]
            self.R32[form], self.M32[form] = float(ratio.max()), float(ratio.mean())

    @property
    def rows(self):
        return self.d.rows

    def bounds(self, form):
        """(lo, hi, resolved, clamped) [rows, 64]; clamped: the interval reaches down to the 1e-10 floor"""
        T = 4 * self.R32[form] * self.u
        sc = self.scale.astype(np.float64)
        raw = 10 * np.log10(np.maximum(self.P64, FLOOR))
        dd = 4 * E * np.maximum(np.abs(raw), 1) * np.abs(sc)
        a, b = db64(self.P64 - T, self.scale, self.shift), db64(self.P64 + T, self.scale, self.shift)
        return np.minimum(a, b) - dd, np.maximum(a, b) + dd, T <= 1e-2 * np.maximum(self.P64, FLOOR), self.P64 - T <= FLOOR

    def resolved_by_clip(self, form):
        """[(kind, resolved share)] per clip"""
        res = self.bounds(form)[2].reshape(self.d.B, -1)
        return [(k, float(res[b].mean())) for b, k in enumerate(self.d.kinds)]


@functools.lru_cache(maxsize=None)
def ref(table_name, max_band, shape, bn):
    return Ref(table_name, max_band, shape, bn)


# ------------------------------------------------------------------------------------------------ buffers
def wave_buffer(wav, offset):
    """flat float32 torch tensor [guard | B * N | guard] of NaN guards, and the interior's first element.  `offset` 1 puts the
    interior 4 bytes past an 8-byte boundary of a buffer that itself starts on one."""
    lead = WAVE_GUARD + offset
    buf = nan_rows(1, lead + wav.size + WAVE_GUARD, torch.float32).reshape(-1)
    buf[lead: lead + wav.size] = torch.from_numpy(wav.reshape(-1))
    return buf, lead


def out_buffer(rows):
    return nan_rows(rows + GUARD, BANDS, torch.float32)


def as_output(db):
    """what a kernel that computes `db` [rows, 64] exactly would leave in out_buffer"""
    return torch.cat([torch.from_numpy(np.asarray(db, dtype=np.float64)).to(torch.float32), nan_rows(GUARD, BANDS, torch.float32)])


# ------------------------------------------------------------------------------------------------ the checker
def _where(bad, what, got, want):
    idx = np.argwhere(bad)
    i, m = idx[0]
    return (f"{what}: {idx.shape[0]} of {bad.size} elements are off, the first at row {i}, band {m}: "
            f"{float(got[i, m])!r}, float64 says {float(want[i, m])!r}")


def measure(r, full, form):
    """figures of `full` [rows + GUARD, 64] float32 (torch) against case `r`, nothing asserted but the buffer's shape"""
    assert full.dtype == torch.float32 and tuple(full.shape) == (r.rows + GUARD, BANDS), f"{r.what}: buffer {tuple(full.shape)} {full.dtype}"
    got = full[: r.rows].numpy()
    lo, hi, resolved, clamped = r.bounds(form)
    fig = dict(what=f"{r.what}-form{form}", R32=r.R32[form], M32=r.M32[form], guards=guards_intact(full, r.rows))
    fig["finite"] = np.isfinite(got)
    g = got.astype(np.float64)
    fig["outside"] = ~((g >= lo) & (g <= hi)) | ~fig["finite"]
    # how far towards its side's end of the interval the value sits (1 = on it), over the elements whose interval is not clamped
    with np.errstate(invalid="ignore", divide="ignore"):
        side = np.where(g >= r.db64, (g - r.db64) / (hi - r.db64), (r.db64 - g) / (r.db64 - lo))
    sel = ~clamped & fig["finite"]
    fig["max ratio"] = float(side[sel].max()) if sel.any() else 0.0
    fig["resolved share"] = float(resolved.mean())
    err, err32 = np.abs(g - r.db64)[resolved], np.abs(r.db32[form].astype(np.float64) - r.db64)[resolved]
    fig["mean got"], fig["mean restated"] = (float(err.mean()), float(err32.mean())) if resolved.any() else (0.0, 0.0)
    fig["mean ratio"] = fig["mean got"] / fig["mean restated"] if fig["mean restated"] > 0 else (0.0 if fig["mean got"] == 0 else float("inf"))
    fig["silent off"] = np.zeros_like(fig["outside"])
    fig["silent off"][r.d.silent] = (got[r.d.silent] != r.silent_value[0][None]) & (got[r.d.silent] != r.silent_value[1][None])
    return fig


def check(r, full, form):
    """raises AssertionError naming the case, the first bad row and band and the number of bad elements; returns the figures"""
    fig = measure(r, full, form)
    what, got = fig["what"], full[: r.rows].numpy()
    print(f"{what}: R32 = {fig['R32']:.2f}, M32 = {fig['M32']:.3f}, max |got - dB64| / its side of the interval = {fig['max ratio']:.4f}, "
          f"mean |got - dB64| / mean |restated - dB64| = {fig['mean ratio']:.3f} over the resolved {100 * fig['resolved share']:.2f} %")
    assert fig["R32"] <= R32_MAX, f"{what}: the float32 restatement itself is {fig['R32']:.1f} u from float64 (at most {R32_MAX:.0f})"
    assert fig["guards"], f"{what}: guard rows written"
    assert bool(fig["finite"].all()), _where(~fig["finite"], what + " (not finite)", got, r.db64)
    assert not fig["outside"].any(), _where(fig["outside"], what + " (outside the interval)", got, r.db64)
    assert fig["mean ratio"] <= 2, (f"{what}: mean |got - dB64| = {fig['mean got']:.3e} is {fig['mean ratio']:.3f} x the restatement's "
                                    f"{fig['mean restated']:.3e} (at most 2)")
    assert not fig["silent off"].any(), _where(fig["silent off"], what + " (a silent frame is not -100 scale + shift)", got, r.db64)
    return fig
