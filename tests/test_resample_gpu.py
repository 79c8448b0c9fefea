"""The resampling kernel (csrc/resample.hip), WaveResampler and SpeedPerturb on the GPU against the float64 rule of
tests/resample_ref.py.

Impulses: rows of +-32767 on a comb wider than the widest phase, shifted by one sample per row over a whole period, put at most one
non-zero term under every output and meet every (phase, tap) pair; the output must then be float32(float32(w) * x) exactly.  That is
the comparison that sees a dropped or shifted edge tap: an edge weight is 1e-6 of a sum of noise.
Noise: per output, |y - y64| <= (taps + 4) 2^-24 S[k], S[k] = sum_j |w x| and taps the bank's widest tap count: the dot-product bound
for any summation order plus one rounding each for the weight, the input conversion and the store.  Derived, not measured; the
float32 restatement of the reference reaches about 5 of those units, 17 to 41 are allowed.
Everything that is a matter of which sample sits where -- tile positions, batches, strides, alignment, length dtypes -- is compared
bit for bit.
`python tests/test_resample_gpu.py OUT.json` writes the worst units of the noise cases of a run (tests/golden/resample_measured.json)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = os.path.join(HERE, "golden", "resample_measured.json")
PAIRS = [(3, 1), (1, 2), (2, 1), (441, 160), (441, 320), (160, 147), (11, 10), (9, 10)]
DTYPES = [np.int16, np.float32]
IDS = lambda p: "%d-%d" % p if isinstance(p, tuple) else np.dtype(p).name


def resampler(pair):
    from fbk_fairseq_st_amd.resample import WaveResampler
    return WaveResampler(*pair)


def batch(rows, extra=37):
    """rows of one dtype -> (device waves [B, Nmax] with Nmax odd and 32767 / NaN behind every length, lengths, the host buffer)"""
    dt = rows[0].dtype
    nmax = max(len(r) for r in rows) + extra
    nmax += 1 - nmax % 2
    buf = np.full((len(rows), nmax), 32767 if dt == np.int16 else np.nan, dtype=dt)
    for b, r in enumerate(rows):
        buf[b, :len(r)] = r
    return torch.from_numpy(buf).to(DEV), torch.tensor([len(r) for r in rows], device=DEV), buf


def run(rs, rows, **kw):
    waves, lens, buf = batch(rows, **kw)
    out = rs.resample(waves, lens)
    torch.cuda.synchronize()
    assert out["waves"].dtype == torch.float32 and out["lengths"].dtype == torch.int64 and out["status"].dtype == torch.int32
    assert out["waves"].shape[1] == rs.num_samples(waves.shape[1])
    return out["waves"].cpu().numpy(), out["lengths"].tolist(), out["status"].tolist(), buf


def noise(n, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.int16:
        return rng.integers(-32768, 32768, n).astype(np.int16)       # full scale
    return rng.standard_normal(n).astype(np.float32)


def tile_of(rs):
    from fbk_fairseq_st_amd import kernels as K
    iu, ou, taps, _, _, _, extra = rs.tables("cpu")[0][0].tolist()
    return K.resample_tile(iu, ou, extra)


def noise_lengths(rs):
    """input lengths whose output counts sit at tile - 1, tile, tile + 1 and 2 tile + 1 (the nearest count an upsampling can give),
    and 1, 2, half a tap width, one whole in_unit and one either side: windows that run off both ends"""
    iu, ou, taps = rs.bank["in_unit"], rs.bank["out_unit"], rs.bank["taps"]
    tile = tile_of(rs)
    lens = [-(-t * iu // ou) for t in (tile - 1, tile, tile + 1, 2 * tile + 1)]
    counts = [rs.num_samples(n) for n in lens]
    assert counts[0] <= tile <= counts[1] and tile < counts[2] <= tile + max(1, -(-ou // iu)) + 1 and counts[3] > 2 * tile
    return lens + [1, 2, max(1, taps // 2), max(1, iu - 1), iu, iu + 1]


_IMPULSE, _NOISE = {}, {}


def impulse_case(pair, dtype):
    """(rows, n, the kernel's outputs [P, Mmax], lengths, statuses), once"""
    key = (pair, np.dtype(dtype).name)
    if key not in _IMPULSE:
        rows, n = R.impulse_rows(*pair, dtype)
        y, ln, st, _ = run(resampler(pair), list(rows))
        _IMPULSE[key] = (rows, n, y, ln, st)
    return _IMPULSE[key]


def noise_case(pair, dtype):
    """(the host buffer with its junk, lengths, the kernel's outputs, lengths out, statuses), once"""
    key = (pair, np.dtype(dtype).name)
    if key not in _NOISE:
        rs = resampler(pair)
        lens = noise_lengths(rs)
        rows = [noise(n, dtype, 11 + b) for b, n in enumerate(lens)]
        y, ln, st, buf = run(rs, rows)
        _NOISE[key] = (buf, lens, y, ln, st)
    return _NOISE[key]


def noise_units(pair, dtype, **twin):
    """per row, the error of the kernel's output in 2^-24 S[k] against the rule (or a twin of it); inf where the lengths differ"""
    buf, lens, y, ln, st = noise_case(pair, dtype)
    worst = []
    for b, n in enumerate(lens):
        y64, S = R.resample(buf[b], n, *pair, **twin)
        if len(y64) != ln[b]:
            worst.append(np.inf)
            continue
        u = R.units(y[b, :ln[b]], y64, S)
        worst.append(float(np.where(np.isnan(u), np.inf, u).max()))
    return worst


# ------------------------------------------------------------------ 1. impulse combs, bit for bit
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_impulse_combs_bit_for_bit(pair, dtype):
    rows, n, y, ln, st = impulse_case(pair, dtype)
    m = R.num_samples(n, *pair)
    assert ln == [m] * len(rows) and st == [0] * len(rows)
    seen = 0
    for b, row in enumerate(rows):
        want = R.impulse_expected(row, n, *pair)
        seen += int((want != 0).sum())
        assert np.array_equal(y[b, :m], want), (b, int(np.argmax(y[b, :m] != want)))
        assert (y[b, m:] == 0).all()
    assert seen > 0


# ------------------------------------------------------------------ 2. noise against float64, per element
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_noise_against_float64(pair, dtype):
    buf, lens, y, ln, st = noise_case(pair, dtype)
    assert ln == [R.num_samples(n, *pair) for n in lens] and st == [0] * len(lens)
    assert np.isfinite(y).all(), "what lies behind a length never reaches an output"
    for b, m in enumerate(ln):
        assert (y[b, m:] == 0).all()
    worst, allowed = noise_units(pair, dtype), R.allowed(*pair)
    print("%d -> %d %s: worst error %.2f of 2^-24 S[k], %.0f allowed" % (pair + (np.dtype(dtype).name, max(worst), allowed)))
    assert max(worst) <= allowed, (worst, allowed)


# ------------------------------------------------------------------ 3. lengths and statuses
@pytest.mark.parametrize("pair", [(3, 1), (1, 2), (441, 160), (11, 10)], ids=IDS)
def test_every_length_up_to_three_units(pair):
    rs = resampler(pair)
    iu = rs.bank["in_unit"]
    lens = list(range(3 * iu + 6))
    x = noise(lens[-1], np.int16, 2)
    waves, _, _ = batch([x], extra=0)
    nmax = waves.shape[1]
    lens.append(nmax)
    out = rs.resample(waves.expand(len(lens), nmax), torch.tensor(lens, device=DEV, dtype=torch.int32))
    want = [R.num_samples(n, *pair) for n in lens]
    assert out["lengths"].tolist() == want and out["status"].tolist() == [1] + [0] * (len(lens) - 1)
    y = out["waves"].cpu().numpy()
    assert y.shape[1] == want[-1]
    cols = np.arange(y.shape[1])[None, :]
    assert (y[cols >= np.array(want)[:, None]] == 0).all(), "zeros behind every length"
    for b in (1, 2, iu - 1, iu, 2 * iu + 1, 3 * iu + 5):    # rows shorter than a window: zeros either side of the samples
        y64, S = R.resample(x, lens[b], *pair)
        assert (R.units(y[b, :want[b]], y64, S) <= R.allowed(*pair)).all(), b


def test_refusals_beside_ordinary_rows():
    from fbk_fairseq_st_amd import kernels as K
    from fbk_fairseq_st_amd.resample import SpeedPerturb
    sp = SpeedPerturb(("9/10", 1, "11/10"))
    x = [noise(1500, np.float32, s) for s in range(8)]
    waves, _, _ = batch(x)
    nmax = waves.shape[1]
    good = sp.apply(waves, [1500] * 8, 0, choice=[0, 1, 2, 0, 1, 2, 0, 1])
    lens = torch.tensor([-1, 1500, nmax + 1, 1500, 0, 1500, 1500, 1500], device=DEV)
    choice = [0, 1, 2, 0, 1, 2, -1, 3]
    out = sp.apply(waves, lens, 0, choice=choice)
    assert out["status"].tolist() == [2, 0, 2, 0, 1, 0, 2, 2] and out["choice"].tolist() == choice
    assert out["lengths"].tolist() == [0, 1500, 0, sp.num_samples(1500, 0), 0, sp.num_samples(1500, 2), 0, 0]
    for b in range(8):
        if out["status"][b] == 0:
            assert torch.equal(out["waves"][b], good["waves"][b]), "an ordinary row beside refused ones"
        else:
            assert out["waves"][b].eq(0).all()
    assert torch.isfinite(out["waves"]).all()
    # a result narrower than a row's samples: that row is refused, the others are what they were
    banks, first, weights = sp.tables(DEV)
    narrow = sp.num_samples(1500, 1)                # 1,500: the rows of the slow factor give 1,667
    y, ln, st = K.resample(waves, torch.full((8,), 1500, device=DEV), banks, first, weights, narrow, ratio_id=good["choice"])
    assert st.tolist() == [2, 0, 0, 2, 0, 0, 2, 0] and ln.tolist() == [0, 1500, 1364, 0, 1500, 1364, 0, 1500]
    for b in range(8):
        assert torch.equal(y[b], good["waves"][b, :narrow] if st[b] == 0 else torch.zeros_like(y[b]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nothing_is_written_outside_the_results(dtype):
    """the entry point itself on sentinel-filled buffers with guards either side"""
    from fbk_fairseq_st_amd import lib as L
    from fbk_fairseq_st_amd.resample import SpeedPerturb
    sp = SpeedPerturb(("9/10", 1, "441/160"))
    banks, first, weights = sp.tables(DEV)
    lens = [2000, 0, 1999, 2500, 7, -5]
    rid = [0, 1, 2, 2, 0, 1]
    waves, _, buf = batch([noise(2500, dtype, s) for s in range(6)])
    B, nmax = waves.shape
    mmax, G = sp.num_samples(nmax), 64
    out = torch.full((G + B * mmax + G,), -7.0, device=DEV)
    out_len = torch.full((G + B + G,), -7, dtype=torch.int64, device=DEV)
    status = torch.full((G + B + G,), -7, dtype=torch.int32, device=DEV)
    lens_t = torch.tensor(lens, device=DEV)
    rid_t = torch.tensor(rid, dtype=torch.int32, device=DEV)
    before = waves.clone()
    L.check(L.load().s2t_resample(waves.data_ptr(), waves.element_size(), nmax, lens_t.data_ptr(), 8, rid_t.data_ptr(), B, nmax, mmax,
                                  banks.data_ptr(), banks.shape[0], first.data_ptr(), first.shape[0], weights.data_ptr(), weights.shape[0],
                                  out[G:].data_ptr(), out_len[G:].data_ptr(), status[G:].data_ptr(), L.stream()), "s2t_resample")
    torch.cuda.synchronize()
    for t in (out, out_len, status):
        assert t[:G].eq(-7).all() and t[-G:].eq(-7).all(), "the guards"
    assert torch.equal(waves.view(torch.int32 if dtype == np.float32 else torch.int16), before.view(torch.int32 if dtype == np.float32 else torch.int16))
    pairs = [(9, 10), (1, 1), (441, 160)]
    want = [R.num_samples(n, *pairs[r]) if n >= 0 else 0 for n, r in zip(lens, rid)]
    assert out_len[G:G + B].tolist() == want and status[G:G + B].tolist() == [0, 1, 0, 0, 0, 2]
    y = out[G:G + B * mmax].view(B, mmax).cpu().numpy()
    for b in range(B):
        assert (y[b, want[b]:] == 0).all() and np.isfinite(y[b]).all()
        if want[b]:
            y64, S = R.resample(buf[b], lens[b], *pairs[rid[b]])
            assert (R.units(y[b, :want[b]], y64, S) <= R.allowed(*pairs[rid[b]])).all()


# ------------------------------------------------------------------ 4. orig == new
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_equal_rates_copy_bit_for_bit(dtype):
    rs = resampler((16000, 16000))
    lens = [0, 1, 2047, 2048, 2049, 4097]
    rows = [noise(n, dtype, 40 + n % 7) for n in lens]
    y, ln, st, buf = run(rs, rows)
    assert ln == lens and st == [1, 0, 0, 0, 0, 0] and y.shape[1] == buf.shape[1]
    for b, n in enumerate(lens):
        assert np.array_equal(y[b, :n], rows[b].astype(np.float32)) and (y[b, n:] == 0).all()


# ------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_row_alone_and_inside_a_mixed_batch(dtype):
    from fbk_fairseq_st_amd.resample import SpeedPerturb
    factors = ("9/10", 1, "11/10", "441/160", "3", "1/2")
    sp = SpeedPerturb(factors)
    lens = [3000, 2999, 3001, 5000, 4321, 1234, 2500, 17]
    choice = [0, 1, 2, 3, 4, 5, 3, 2]
    rows = [noise(n, dtype, 70 + b) for b, n in enumerate(lens)]
    waves, lens_t, _ = batch(rows)
    out = sp.apply(waves, lens_t, 3, choice=choice)
    assert out["status"].tolist() == [0] * 8
    for b, c in enumerate(choice):
        alone = resampler(sp.pairs[c]).resample(waves[b:b + 1], lens_t[b:b + 1])
        m = int(alone["lengths"][0])
        assert m == int(out["lengths"][b]) == R.num_samples(lens[b], *sp.pairs[c])
        assert torch.equal(alone["waves"][0, :m], out["waves"][b, :m]) and out["waves"][b, m:].eq(0).all(), (b, c)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pair", [(3, 1), (441, 160), (1, 2), (11, 10)], ids=IDS)
def test_tile_position_stride_alignment_and_length_dtype(pair, dtype):
    rs = resampler(pair)
    iu, ou = rs.bank["in_unit"], rs.bank["out_unit"]
    tile = tile_of(rs)
    n = -(-(tile + 300) * iu // ou)
    x = noise(n, dtype, 90)
    ref, ln, st, _ = run(rs, [x])
    m = ln[0]
    assert st == [0] and m > tile
    # another tile position: whole units of zeros in front move every output by as many units
    for units in (1, 5):
        moved, ln2, _, _ = run(rs, [np.concatenate([np.zeros(units * iu, dtype), x])])
        assert ln2 == [m + units * ou] and np.array_equal(moved[0, units * ou:ln2[0]], ref[0, :m]), units
    # another row stride, an odd element offset of the base, int32 lengths
    wide = torch.from_numpy(np.stack([np.concatenate([noise(1, dtype, 1), x, noise(12, dtype, 2)])] * 3)).to(DEV)
    for view in (wide[:, 1:1 + n], wide[:, 1:1 + n + 7], wide[1:2, 1:1 + n]):
        for ldt in (torch.int32, torch.int64):
            out = rs.resample(view, torch.full((view.shape[0],), n, dtype=ldt, device=DEV))
            assert out["lengths"].tolist() == [m] * view.shape[0]
            for b in range(view.shape[0]):
                assert np.array_equal(out["waves"][b, :m].cpu().numpy(), ref[0, :m])


# ------------------------------------------------------------------ 6. the classes
def test_wave_resampler_against_the_reference_and_into_the_front_end():
    from fbk_fairseq_st_amd.fbank import FbankFrontEnd
    rs = resampler((48000, 16000))
    t = np.arange(9000) / 48000.0
    rows = [np.rint(8000 * np.sin(2 * np.pi * 440.0 * t) + noise(9000, np.float32, 5) * 500).astype(np.int16)[:n] for n in (9000, 6001, 4800)]
    y, ln, st, buf = run(rs, rows)
    assert ln == [3000, 2001, 1600] and st == [0, 0, 0]
    for b, n in enumerate((9000, 6001, 4800)):
        y64, S = R.resample(buf[b], n, 48000, 16000)
        assert (R.units(y[b, :ln[b]], y64, S) <= R.allowed(48000, 16000)).all()
    # a 1 kHz unit sine, away from the edges (the float64 rule itself is 3.99e-4 away: tests/test_resample_ref_cpu.py)
    tone = np.sin(2 * np.pi * 1000.0 * np.arange(4800) / 48000.0).astype(np.float32)
    z, lz, _, _ = run(rs, [tone])
    assert lz == [1600] and np.abs(z[0, :1600] - np.sin(2 * np.pi * 1000.0 * np.arange(1600) / 16000.0))[20:-20].max() <= 1e-3
    # straight into the filterbanks: the same features as from a fresh contiguous tensor of the same samples
    waves, lens, _ = batch(rows)
    out = rs.resample(waves, lens)
    fe = FbankFrontEnd()
    a = fe.features(out["waves"], out["lengths"])
    b = fe.features(out["waves"].clone(memory_format=torch.contiguous_format), out["lengths"].clone())
    assert a["lengths"].tolist() == [fe.num_frames(m) for m in ln] and a["status"].tolist() == [0, 0, 0]
    assert torch.equal(a["features"], b["features"]) and torch.equal(a["lengths"], b["lengths"])


def test_speed_perturb_equals_per_row_resamplers():
    from fbk_fairseq_st_amd.resample import SpeedPerturb
    sp = SpeedPerturb()
    lens = [4000, 3999, 3601, 2000, 1, 3300]
    rows = [noise(n, np.int16, 30 + b) for b, n in enumerate(lens)]
    waves, lens_t, _ = batch(rows)
    choice = [0, 1, 2, 2, 0, 1]
    out = sp.apply(waves, lens_t, update=4, choice=choice)
    assert out["waves"].shape[1] == sp.num_samples(waves.shape[1]) == R.num_samples(waves.shape[1], 9, 10)
    for b, c in enumerate(choice):
        alone = resampler(sp.pairs[c]).resample(waves[b:b + 1], lens_t[b:b + 1])
        m = int(alone["lengths"][0])
        assert m == int(out["lengths"][b]) and torch.equal(alone["waves"][0, :m], out["waves"][b, :m]) and out["waves"][b, m:].eq(0).all()
    drawn = sp.apply(waves, lens_t, update=4)
    assert drawn["choice"].tolist() == sp.draw(6, 4).tolist() and drawn["status"].tolist() == [0] * 6
    assert drawn["lengths"].tolist() == [sp.num_samples(n, c) for n, c in zip(lens, drawn["choice"].tolist())]


# ------------------------------------------------------------------ 7. twins
@pytest.mark.parametrize("twin", sorted(R.TWINS))
def test_twins_fail_where_the_kernel_passes(twin):
    kw, pair = R.TWINS[twin], (441, 160)
    if twin == "outermost_tap_dropped":
        rows, n, y, ln, st = impulse_case(pair, np.int16)
        right = all(np.array_equal(y[b, :ln[b]], R.impulse_expected(r, n, *pair)) for b, r in enumerate(rows))
        wrong = all(np.array_equal(y[b, :ln[b]], R.impulse_expected(r, n, *pair, **kw)) for b, r in enumerate(rows))
        assert right and not wrong
        return
    allowed = R.allowed(*pair)
    assert max(noise_units(pair, np.int16)) <= allowed
    assert max(noise_units(pair, np.int16, **kw)) > allowed, "the kernel is not within the bound of the wrong rule"


# ------------------------------------------------------------------ 8. the measured record
def test_measured_record_lies_inside_the_bound():
    with open(MEASURED) as f:
        rec = json.load(f)
    assert sorted(rec["worst_units"]) == sorted("%d-%d %s" % (p + (np.dtype(d).name,)) for p in PAIRS for d in DTYPES)
    for key, worst in rec["worst_units"].items():
        pair = tuple(int(v) for v in key.split()[0].split("-"))
        assert 0.0 < worst <= R.allowed(*pair), key


def main(path):
    rec = {"what": "worst |y - y64| / (2^-24 S[k]) of the noise cases of tests/test_resample_gpu.py per pair and input dtype, on an MI355X; "
                   "allowed: taps + 4", "worst_units": {}, "allowed": {}}
    for pair in PAIRS:
        for dtype in DTYPES:
            key = "%d-%d %s" % (pair + (np.dtype(dtype).name,))
            rec["worst_units"][key] = round(max(noise_units(pair, dtype)), 3)
            rec["allowed"][key] = R.allowed(*pair)
            print(key, rec["worst_units"][key], rec["allowed"][key])
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))                        # the package, when this file is run as a script
    main(sys.argv[1])
