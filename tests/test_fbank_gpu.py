"""The filterbank and normalisation kernels (csrc/fbank.hip) and FbankFrontEnd on the GPU against the float64 rule of
tests/fbank_ref.py.

Log-mel tolerance: per case and per mel bin, the kernel's worst error over the frames against float64 is at most
8 x max(the float32 host restatement's worst error on that bin, 2e-6) -- the lowest bins hold one FFT bin that DC removal and
pre-emphasis attenuate by about 30 dB, where the float32 restatement itself is off by 1e-4 to 1e-3; every case has at least 100
frames.  Everything that is a matter of which frame sits where -- utterance lengths, tile edges, batches, row strides, alignment,
input dtype -- is compared bit for bit against the frames of a call that is held to the bound.
CMVN: against float64 CMVN of the very float32 values the kernel was given, within 1e-4 max(1, |ref|), on columns with a standard
deviation of at least 0.1; constant columns exactly 0.
`python tests/test_fbank_gpu.py OUT.json` writes the worst ratios and errors of a run (tests/golden/fbank_measured.json)."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import fbank_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = os.path.join(HERE, "golden", "fbank_measured.json")
LOG_FLOOR = np.float32(math.log(2.0 ** -23))
WORST = {}                            # (input dtype, N) -> [worst err / max(yardstick, 2e-6), worst absolute error]
NAMES = dict(sr="sample_rate")


def front(cfg, normalize=False):
    from fbk_fairseq_st_amd.fbank import FbankFrontEnd
    return FbankFrontEnd(normalize=normalize, **{NAMES.get(k, k): v for k, v in cfg.items()})


def batch(rows, extra=37):
    """rows of one dtype -> (device waves [B, Nmax] with Nmax odd and 32767 / NaN behind every length, lengths)"""
    dt = rows[0].dtype
    nmax = max(len(r) for r in rows) + extra
    nmax += 1 - nmax % 2
    buf = np.full((len(rows), nmax), 32767 if dt == np.int16 else np.nan, dtype=dt)
    for b, r in enumerate(rows):
        buf[b, :len(r)] = r
    return torch.from_numpy(buf).to(DEV), torch.tensor([len(r) for r in rows], device=DEV)


def run(fe, rows, **kw):
    out = fe.features(*batch(rows, **kw))
    torch.cuda.synchronize()
    assert out["features"].dtype == torch.float32 and out["lengths"].dtype == torch.int64 and out["status"].dtype == torch.int32
    return out["features"].cpu().numpy(), out["lengths"].tolist(), out["status"].tolist()


_GOT = {}


def case_features(case):
    """the kernel's features of a case's utterance (alone in its batch), once"""
    if case["name"] not in _GOT:
        x = R.case_refs(case)[0]
        f, n, st = run(front(case["cfg"]), [x])
        assert n == [case["frames"]] and st == [0] and (f[0, n[0]:] == 0).all()
        _GOT[case["name"]] = f[0, :n[0]]
    return _GOT[case["name"]]


# ------------------------------------------------------------------ the rule, within the bound
@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_cases_against_float64(case):
    x, r64, r32 = R.case_refs(case)
    got = case_features(case)
    assert got.shape == r64.shape and np.isfinite(got).all()
    err, bound = R.compare(got, r64, r32)
    ratio = float((err / (bound / R.FACTOR)).max())
    print("%s: worst error %.3g, worst ratio to the yardstick %.3g (bound %g)" % (case["name"], err.max(), ratio, R.FACTOR))
    key = ("int16" if x.dtype == np.int16 else "float32", R.geometry(case["cfg"].get("sr", 16000), case["cfg"].get("frame_length", 25.0), 10.0)[2])
    w = WORST.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], ratio), max(w[1], float(err.max()))
    assert (err <= bound).all(), (case["name"], int(np.argmax(err / bound)), float((err / bound).max()))


@pytest.mark.parametrize("twin", sorted(t for t in R.FBANK_TWINS if t != "floor_1e-10"))
def test_twins_fail_where_the_kernel_passes(twin):
    case = R.CASES[7] if twin == "first_sample_not_emphasised" else R.CASES[0]
    assert R.twin_applies(twin, case["cfg"])
    x, r64, r32 = R.case_refs(case)
    got = case_features(case)
    wrong = R.fbank(x, **dict(case["cfg"], **R.FBANK_TWINS[twin]))
    err, bound = R.compare(got, r64, r32)
    terr, _ = R.compare(wrong, r64, r32)
    away, _ = R.compare(got, wrong, r32)
    assert (err <= bound).all() and (terr > bound).any() and (away > bound).any()


def test_silence_and_a_constant_are_exactly_the_floor():
    for cfg in (dict(), dict(sr=8000, num_mel_bins=23), dict(sr=22050, num_mel_bins=128)):
        fe = front(cfg)
        n = fe.W + 7 * fe.S
        f, ln, st = run(fe, [np.zeros(n, np.int16), np.full(n, 1234, np.int16), np.full(n, -32768, np.int16)])
        assert ln == [8, 8, 8] and st == [0, 0, 0] and (f == LOG_FLOOR).all()
        f, _, _ = run(fe, [np.zeros(n, np.float32)])
        assert (f == LOG_FLOOR).all()
    floor = R.fbank(np.zeros(1000, np.int16), dtype=np.float32)
    wrong = R.fbank(np.zeros(1000, np.int16), dtype=np.float32, **R.FBANK_TWINS["floor_1e-10"])
    assert (floor == LOG_FLOOR).all() and (wrong != LOG_FLOOR).all()


def test_a_batch_too_short_for_any_frame():
    for normalize in (False, True):
        out = front(dict(), normalize).features(torch.full((3, 399), 7, dtype=torch.int16, device=DEV), torch.tensor([399, 0, 400], device=DEV))
        assert tuple(out["features"].shape) == (3, 0, 80) and out["lengths"].tolist() == [0, 0, 0] and out["status"].tolist() == [1, 1, 2]


# ------------------------------------------------------------------ which frame sits where: bit for bit
SR_CASES = [R.CASES[0], R.CASES[2], R.CASES[3]]                     # 16 kHz / N = 512, 8 kHz / 256, 22.05 kHz / 1024


@pytest.mark.parametrize("case", SR_CASES, ids=[c["name"] for c in SR_CASES])
def test_utterance_lengths_tile_edges_and_statuses(case):
    from fbk_fairseq_st_amd import kernels as K
    x = R.case_refs(case)[0]
    full = case_features(case)
    fe = front(case["cfg"])
    W, S, ft = fe.W, fe.S, K.fbank_frame_tile(fe.N)
    frames = [ft - 1, ft, ft + 1, 2 * ft, 2 * ft + 1, 120]
    lens = [W - 1, W, W + S - 1, W + S, 0] + [W + (m - 1) * S for m in frames] + [W + (ft - 1) * S + S - 1]
    want = [0, 1, 1, 2, 0] + frames + [ft]
    assert [fe.num_frames(n) for n in lens] == want
    f, ln, st = run(fe, [x[:n] for n in lens])
    assert ln == want and st == [1, 0, 0, 0, 1] + [0] * 7
    for b, m in enumerate(want):
        assert np.array_equal(f[b, :m], full[:m]), (b, m)
        assert (f[b, m:] == 0).all(), "the padding is zeros"
    # statuses 1 and 2 beside ordinary sentences, lengths beyond the padded width
    waves, _ = batch([x[:W + 3 * S], x[:W + 3 * S], x[:W + 3 * S], x[:W + 3 * S]])
    out = fe.features(waves, torch.tensor([-1, W + 3 * S, waves.shape[1] + 1, W - 1], device=DEV))
    assert out["status"].tolist() == [2, 0, 2, 1] and out["lengths"].tolist() == [0, 4, 0, 0]
    got = out["features"].cpu().numpy()
    assert np.array_equal(got[1, :4], full[:4]) and (got[[0, 2, 3]] == 0).all() and (got[1, 4:] == 0).all()
    nrm = front(case["cfg"], normalize=True).features(waves, torch.tensor([W, W + S, W + 3 * S, waves.shape[1] + 1], device=DEV))
    assert nrm["status"].tolist() == [1, 0, 0, 2] and nrm["lengths"].tolist() == [0, 2, 4, 0], "one frame has no variance"
    assert (nrm["features"][0] == 0).all() and (nrm["features"][3] == 0).all() and torch.isfinite(nrm["features"]).all()


@pytest.mark.parametrize("case", SR_CASES + [R.CASES[-1]], ids=[c["name"] for c in SR_CASES + [R.CASES[-1]]])
def test_same_frame_at_two_tile_positions_and_in_any_batch(case):
    x = R.case_refs(case)[0]
    full = case_features(case)
    fe = front(case["cfg"])
    shifts = [1, 3, 5, 17]
    f, ln, _ = run(fe, [x[k * fe.S:] for k in shifts])
    for b, k in enumerate(shifts):
        assert ln[b] == 120 - k and np.array_equal(f[b, :120 - k], full[k:]), k
    rng = np.random.default_rng(11)
    others = [R.signal(case["kind"], int(rng.integers(fe.W, len(x) + 1)), 100 + i, case["cfg"].get("sr", 16000)) for i in range(15)]
    f16, ln16, _ = run(fe, others[:7] + [x] + others[7:])
    assert ln16[7] == 120 and np.array_equal(f16[7, :120], full) and (f16[7, 120:] == 0).all(), "alone and inside a batch of 16"


def test_input_dtype_alignment_and_strides():
    case = R.CASES[0]
    x = R.case_refs(case)[0]
    full = case_features(case)
    fe = front(case["cfg"])
    n = len(x)
    lens = torch.tensor([n, n - 161, n - 1000], device=DEV)
    for dt, junk in ((torch.int16, 32767), (torch.float32, float("nan"))):
        xs = torch.from_numpy(x.astype(np.float32) if dt == torch.float32 else x).to(DEV)
        ld = n + 3 + n % 2                                          # an odd row stride
        assert ld % 2 == 1
        flat = torch.full((3 * ld + 8,), junk, dtype=dt, device=DEV)
        rows = flat[1:].as_strided((3, n), (ld, 1))                 # rows 1, 1 + ld, 1 + 2 ld elements into the buffer: element-aligned only
        assert rows.data_ptr() % (2 * flat.element_size()) != 0 and rows[1].data_ptr() % (2 * flat.element_size()) == 0
        for b in range(3):
            rows[b, :int(lens[b])] = xs[:int(lens[b])]
        out = fe.features(rows, lens)
        got = out["features"].cpu().numpy()
        assert out["lengths"].tolist() == [120, 119, 114]
        for b, m in enumerate([120, 119, 114]):
            assert np.array_equal(got[b, :m], full[:m]) and (got[b, m:] == 0).all(), (dt, b)
        wide = torch.full((3, 2 * n + 5), junk, dtype=dt, device=DEV)
        view = wide[:, 3:3 + n]                                     # a strided view of a wider batch
        view[0], view[2, :n - 1000] = xs, xs[:n - 1000]
        out = fe.features(view[::2], lens[::2])
        got = out["features"].cpu().numpy()
        assert np.array_equal(got[0], full) and np.array_equal(got[1, :114], full[:114]) and (got[1, 114:] == 0).all()


def test_raw_entry_point_touches_nothing_but_its_outputs():
    """sentinel-filled outputs with guard rows: every feature row is written, the padding comes back zero, the guards stay"""
    from fbk_fairseq_st_amd import lib as L
    case = R.CASES[2]
    x = R.case_refs(case)[0]
    full = case_features(case)
    fe = front(case["cfg"])
    window, twiddle, bank, weights = fe.tables(DEV)
    waves, lens = batch([x[:fe.W + 40 * fe.S], x[:fe.W - 1], x], extra=200)
    B, nmax = waves.shape
    tmax, F, G = fe.num_frames(nmax), fe.num_mel_bins, 64
    out = torch.full((B * tmax * F + 2 * G,), -777.0, device=DEV)
    meta = torch.full((2, B + 2), -777, dtype=torch.int32, device=DEV)
    rc = L.load().s2t_fbank(waves.data_ptr(), 2, waves.stride(0), lens.data_ptr(), B, nmax, fe.W, fe.S, fe.N, F, tmax, window.data_ptr(),
                            twiddle.data_ptr(), bank.data_ptr(), weights.data_ptr(), weights.numel(), 1, 0.97, out[G:].data_ptr(),
                            meta[0, 1:].data_ptr(), meta[1, 1:].data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert rc == 0 and meta[0].tolist() == [-777, 41, 0, 120, -777] and meta[1].tolist() == [-777, 0, 1, 0, -777]
    assert (out[:G] == -777).all() and (out[-G:] == -777).all()
    got = out[G:-G].view(B, tmax, F).cpu().numpy()
    assert np.array_equal(got[0, :41], full[:41]) and np.array_equal(got[2, :120], full) and (got[0, 41:] == 0).all()
    assert (got[1] == 0).all() and (got[2, 120:] == 0).all() and tmax > 120


# ------------------------------------------------------------------ CMVN
def cmvn_batch(F, lens, seed, tmax=None):
    rng = np.random.default_rng(seed)
    tmax = tmax or max(lens) + 3
    x = np.full((len(lens), tmax, F), np.nan, np.float32)
    for b, m in enumerate(lens):
        x[b, :m] = (rng.normal(15.0, 1.0, (1, F)) + rng.normal(0, 1, (m, F)) * rng.uniform(0.3, 4.0, (1, F))).astype(np.float32)
    return x


@pytest.mark.parametrize("F", [1, 23, 32, 33, 64, 65, 80, 128])
@pytest.mark.parametrize("len_dtype", [torch.int32, torch.int64])
def test_cmvn_against_float64(F, len_dtype):
    from fbk_fairseq_st_amd import kernels as K
    lens = [130, 9, 131, 1000, 33]
    x = cmvn_batch(F, lens, F)
    dev = torch.from_numpy(x).to(DEV)
    out_len, status = K.cmvn(dev, torch.tensor(lens, dtype=len_dtype, device=DEV))
    got = dev.cpu().numpy()
    assert out_len.tolist() == lens and status.tolist() == [0] * len(lens)
    for b, m in enumerate(lens):
        assert x[b, :m].std(0, ddof=1).min() >= 0.1
        ref = R.cmvn(x[b, :m])
        assert R.cmvn_within(got[b, :m], ref).all(), (b, float(np.abs(got[b, :m] - ref).max()))
        assert (got[b, m:] == 0).all(), "the padding is zeros whatever was there"
        if m > 100:
            assert not R.cmvn_within(R.cmvn_biased(x[b, :m]), ref).all(), "the biased twin is outside the bound"


def test_cmvn_constant_columns_the_switch_and_statuses():
    from fbk_fairseq_st_amd import kernels as K
    lens = [200, 200, 1, 0, -1, 204, 2]
    x = cmvn_batch(80, [200, 200, 1, 0, 0, 203, 2], 9, tmax=203)
    x[0, :200, 5], x[0, :200, 79] = 12.625, -3.1                    # constant columns: every column of the utterance takes +1e-8
    x[6, 0], x[6, 1] = 14.0, 16.0
    x[1, :200, 40] = np.where(np.arange(200) % 2 == 0, 5e-5, -5e-5).astype(np.float32)     # variance 2.5e-9: below 1e-8, not zero
    dev = torch.from_numpy(x).to(DEV)
    out_len, status = K.cmvn(dev, torch.tensor(lens, device=DEV))
    got = dev.cpu().numpy()
    assert status.tolist() == [0, 0, 1, 1, 2, 2, 0] and out_len.tolist() == [200, 200, 0, 0, 0, 0, 2]
    assert (got[0, :200, 5] == 0).all() and (got[0, :200, 79] == 0).all(), "a constant column normalises to exactly 0"
    assert np.isfinite(got).all() and (got[2:6] == 0).all() and (got[:2, 200:] == 0).all()
    keep = [c for c in range(80) if c not in (5, 79)]
    assert R.cmvn_within(got[0, :200][:, keep], R.cmvn(x[0, :200])[:, keep]).all()
    ref = R.cmvn(x[1, :200])
    mean, sd = x[1, :200, 40].astype(np.float64).mean(), x[1, :200, 40].astype(np.float64).std(ddof=1)
    plain = (x[1, :200, 40] - mean) / sd
    assert np.abs(ref[:, 40] - plain).max() > 1.5e-4, "the +1e-8 form is visible on this column"
    assert R.cmvn_within(got[1, :200], ref).all() and not R.cmvn_within(plain, ref[:, 40]).all()
    assert R.cmvn_within(got[6, :2], R.cmvn(x[6, :2])).all(), "two frames are enough"


def test_normalised_call_is_cmvn_of_the_plain_call():
    from fbk_fairseq_st_amd import kernels as K
    case = R.CASES[0]
    x = R.case_refs(case)[0]
    waves, lens = batch([x, x[:len(x) // 2], x[:100], x[:front(case["cfg"]).W]])
    plain = front(case["cfg"]).features(waves, lens)
    nrm = front(case["cfg"], normalize=True).features(waves, lens)
    again = plain["features"].clone()
    out_len, status = K.cmvn(again, plain["lengths"])
    assert torch.equal(nrm["features"], again) and torch.equal(nrm["lengths"], out_len.long())
    assert nrm["status"].tolist() == [0, 0, 1, 1] and plain["status"].tolist() == [0, 0, 1, 0]
    alone = front(case["cfg"]).normalize_features(plain["features"], plain["lengths"])
    assert torch.equal(alone["features"], again) and alone["status"].tolist() == [0, 0, 1, 1]
    ref = R.cmvn(plain["features"][0].cpu().numpy())
    assert R.cmvn_within(nrm["features"][0].cpu().numpy(), ref).all()


# ------------------------------------------------------------------ plumbing
def test_net_input_feeds_inference_step():
    """net_input handed to task.inference_step with a CTCDecoder on the tiny --ctc-compress-out model gives what the same features
    give as plain tensors: plumbing, not accuracy"""
    import test_ctc_decode_gpu as TC
    from fbk_fairseq_st_amd import tasks
    from fbk_fairseq_st_amd.ctc_decoder import CTCDecoder
    from fbk_fairseq_st_amd.data import Dictionary
    from fbk_fairseq_st_amd.registry import namespace
    model, sample, meta, _ = TC.tiny_model("model_a")
    src_dict = TC.transcript_dict(meta)
    task = tasks.SpeechTranslationCTCTask(namespace(), Dictionary.synthetic(96), src_dict)
    dec = CTCDecoder(src_dict, strategy="greedy")
    fe = front(dict(), normalize=True)
    waves, lens = batch([R.signal("tone", 16000, 1), R.signal("noise3000", 9000, 2), R.signal("noise30", 12345, 3)])
    ni = fe.net_input(waves, lens)
    assert sorted(ni) == ["src_lengths", "src_tokens"] and ni["src_lengths"].tolist() == [98, 54, 75] and tuple(ni["src_tokens"].shape) == (3, 98, 80)
    model.eval()
    hyps = task.inference_step(dec, [model], {"net_input": ni})
    plain = task.inference_step(dec, [model], {"net_input": {"src_tokens": ni["src_tokens"].clone(), "src_lengths": torch.tensor([98, 54, 75], device=DEV)}})
    assert len(hyps) == len(plain) == 3
    for h, p in zip(hyps, plain):
        assert torch.equal(h[0]["tokens"], p[0]["tokens"]) and torch.equal(h[0]["score"], p[0]["score"])


# ------------------------------------------------------------------ the measured file
def test_measured_file_lies_inside_the_bound():
    """tests/golden/fbank_measured.json: the worst ratios to the yardstick and the worst absolute errors of a run of this file on an
    MI355X, per input dtype and FFT size (written by running the file as a script); the README quotes it.  It sets no bound -- the
    bound is 8 -- but it must lie inside it."""
    with open(MEASURED) as f:
        m = json.load(f)
    assert m["bound"] == R.FACTOR and m["yardstick_floor"] == R.YARD_FLOOR
    keys = sorted(k for k in m if k[0] in "if")
    assert keys == sorted("%s_%d" % (d, n) for d in ("int16", "float32") for n in (256, 512, 1024))
    for k in keys:
        assert 0 < m[k]["worst_ratio"] <= R.FACTOR and 0 < m[k]["worst_error"] < 1e-2, k


def measured():
    out = {"%s_%d" % k: {"worst_ratio": v[0], "worst_error": v[1]} for k, v in sorted(WORST.items())}
    out.update(bound=R.FACTOR, yardstick_floor=R.YARD_FLOOR)
    return out


if __name__ == "__main__":
    rc = pytest.main([os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider"])
    out = sys.modules["test_fbank_gpu"].measured()                   # the module pytest imported holds the run's figures
    out["note"] = ("per input dtype and FFT size, over the cases of tests/test_fbank_gpu.py on an MI355X: the worst ratio of the kernel's "
                   "per-bin error against float64 to max(the float32 host restatement's error on that bin, yardstick_floor), which the "
                   "tests hold to `bound`, and the worst absolute error of a log-mel value")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    sys.exit(int(rc))
