"""The filterbank front end without a GPU: both entry points are exported, bound and refuse bad arguments before anything is
launched, in the order the header states; the limits are the same in the header, in kernels and in the module; the tables are what
the rule says; read_wav reads what the stdlib writes; and the host logic of FbankFrontEnd -- result keys, dtypes, the status merge,
the table cache -- with kernels.fbank / kernels.cmvn replaced by the numpy reference (tests/fbank_ref.py; the kernels have their own
tests)."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch

import fbank_ref as R
from fbk_fairseq_st_amd import fbank as FB
from fbk_fairseq_st_amd import kernels as K
from fbk_fairseq_st_amd import lib as L

FAKE = 1 << 20            # a non-null pointer: a refused call reads and writes nothing
FBANK_ARGS = (("waves", FAKE), ("wave_elem", 2), ("row_stride", 1000), ("lengths", FAKE), ("B", 2), ("Nmax", 1000), ("W", 400), ("S", 160),
              ("N", 512), ("F", 80), ("Tmax", 4), ("window", FAKE), ("twiddle", FAKE), ("bank", FAKE), ("weights", FAKE), ("n_weights", 501),
              ("remove_dc", 1), ("preemph", 0.97), ("out", FAKE), ("out_len", FAKE), ("status", FAKE), ("stream", None))
CMVN_ARGS = (("x", FAKE), ("lengths", FAKE), ("len_elem", 8), ("B", 2), ("Tmax", 10), ("F", 80), ("out_len", FAKE), ("status", FAKE),
             ("stream", None))


def test_exports_bindings_and_limits():
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, args in (("s2t_fbank", FBANK_ARGS), ("s2t_cmvn", CMVN_ARGS)):
        assert name in L.SIGNATURES and hasattr(raw, name) and hasattr(lib, name) and name not in L._SIZE_T_RESULT
        assert len(L.SIGNATURES[name]) == len(args)
    assert lib.s2t_abi_version() == 9
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s2t_hip.h")) as f:
        text = f.read()
    assert "#define S2T_FBANK_MAX_BINS %d" % K.FBANK_MAX_BINS in text and "#define S2T_FBANK_TILE_ELEMS %d" % K.FBANK_TILE_ELEMS in text
    assert K.FBANK_MAX_BINS == 128 == FB.MAX_BINS and K.FBANK_FFT_SIZES == (256, 512, 1024) == FB.FFT_SIZES
    assert [K.fbank_frame_tile(n) for n in K.FBANK_FFT_SIZES] == [32, 16, 8]
    import fbk_fairseq_st_amd
    assert not hasattr(fbk_fairseq_st_amd, "FbankFrontEnd"), "the module is imported by its name"


def check_fbank_refusals(fn):
    f = lambda **kw: fn(*[kw.get(k, d) for k, d in FBANK_ARGS])
    for name in ("waves", "lengths", "window", "twiddle", "bank", "weights", "out", "out_len", "status"):
        assert f(**{name: None}) == -22, name
    for bad in (dict(wave_elem=1), dict(wave_elem=8), dict(Nmax=-1, Tmax=0), dict(row_stride=-1), dict(W=0), dict(S=0), dict(F=0),
                dict(n_weights=-1), dict(Tmax=3), dict(Tmax=5), dict(preemph=-0.1), dict(preemph=1.5), dict(preemph=float("nan"))):
        assert f(**bad) == -22, bad
    for bad in (dict(N=128, W=100, Tmax=6), dict(N=2048, W=1200, Tmax=0), dict(N=500), dict(W=256, Tmax=5), dict(W=513, Tmax=4),
                dict(N=1024, W=512, Tmax=4), dict(F=129), dict(n_weights=513)):
        assert f(**bad) == -95, bad
    # the order: an invalid argument is named before an unsupported one
    assert f(N=2048, F=0) == -22 and f(F=129, wave_elem=3) == -22 and f(W=513, Tmax=99) == -22 and f(N=128, out=None) == -22
    assert f(B=0) == 0 and f(B=-3) == 0 and f(B=0, waves=None, N=7, F=10 ** 6) == 0       # an empty problem: nothing is looked at


def check_cmvn_refusals(fn):
    f = lambda **kw: fn(*[kw.get(k, d) for k, d in CMVN_ARGS])
    for name in ("x", "lengths", "out_len", "status"):
        assert f(**{name: None}) == -22, name
    assert f(len_elem=2) == -22 and f(len_elem=0) == -22 and f(Tmax=-1) == -22 and f(F=0) == -22
    assert f(F=129) == -95 and f(F=129, Tmax=-1) == -22 and f(F=129, x=None) == -22
    assert f(B=0) == 0 and f(B=-1, x=None, F=0) == 0


def test_refusals_before_any_launch_and_their_order():
    check_fbank_refusals(L.load().s2t_fbank)
    check_cmvn_refusals(L.load().s2t_cmvn)


def test_generated_binding_answers_like_ctypes():
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None
    raw = ctypes.CDLL(L.LIB_PATH)
    raw.s2t_fbank.argtypes = L.SIGNATURES["s2t_fbank"]
    raw.s2t_cmvn.argtypes = L.SIGNATURES["s2t_cmvn"]
    for fn in (fast.s2t_fbank, raw.s2t_fbank):
        f = lambda **kw: fn(*[kw.get(k, d) for k, d in FBANK_ARGS])
        assert f(waves=None) == -22 and f(F=129) == -95 and f(preemph=1.5) == -22 and f(row_stride=-(1 << 40)) == -22 and f(B=0) == 0
    check_cmvn_refusals(fast.s2t_cmvn)
    check_cmvn_refusals(raw.s2t_cmvn)


def test_kernels_check_their_operands():
    fe = FB.FbankFrontEnd()
    w, tw, bank, wt = fe.tables("cpu")
    x, n = torch.zeros(2, 1000, dtype=torch.int16), torch.tensor([1000, 500])
    call = lambda *a, **kw: K.fbank(*a, **dict(dict(S=160, N=512), **kw))
    for bad in (lambda: call(x[0], n, w, tw, bank, wt), lambda: call(x.long(), n, w, tw, bank, wt), lambda: call(x, n.int(), w, tw, bank, wt),
                lambda: call(x, n[:1], w, tw, bank, wt), lambda: call(x, n, w[:256], tw, bank, wt), lambda: call(x, n, w.double(), tw, bank, wt),
                lambda: call(x, n, w, tw.float(), bank, wt), lambda: call(x, n, w, tw[:256], bank, wt), lambda: call(x, n, w, tw, bank.long(), wt),
                lambda: call(x, n, w, tw, bank[:0], wt), lambda: call(x, n, w, tw, bank[:, :2], wt), lambda: call(x, n, w, tw, bank, wt.double()),
                lambda: call(x, n, w, tw, bank, torch.zeros(513)), lambda: call(x, n, w, tw, bank, wt, N=300), lambda: call(x, n, w, tw, bank, wt, S=0),
                lambda: call(x, n, w, tw, bank, wt, preemph=1.5)):
        with pytest.raises(ValueError, match="fbank"):
            bad()
    out, out_len, status = call(x[:0], n[:0], w, tw, bank, wt)                 # no sentences: nothing is launched
    assert tuple(out.shape) == (0, 4, 80) and out.dtype == torch.float32 and out_len.dtype == status.dtype == torch.int32
    f = torch.zeros(2, 10, 80)
    for bad in (lambda: K.cmvn(f[0], n), lambda: K.cmvn(f.double(), n), lambda: K.cmvn(f[:, :, ::2], n), lambda: K.cmvn(f, n[:1]),
                lambda: K.cmvn(f, n.float()), lambda: K.cmvn(torch.zeros(2, 10, 129), n), lambda: K.cmvn(torch.zeros(2, 10, 0), n)):
        with pytest.raises(ValueError, match="cmvn"):
            bad()
    out_len, status = K.cmvn(f[:0], n[:0])
    assert tuple(out_len.shape) == (0,) == tuple(status.shape)
    with pytest.raises(L.S2THipError, match="device tensors"):
        call(x, n, w, tw, bank, wt)                                           # a host tensor never reaches a kernel


def test_tables_are_what_the_rule_says():
    for cfg in (dict(), dict(sample_rate=8000, num_mel_bins=23, window_type="hamming"), dict(sample_rate=22050, num_mel_bins=128, window_type="hanning"),
                dict(num_mel_bins=1, low_freq=100.0, high_freq=-500.0), dict(num_mel_bins=40, high_freq=7000.0)):
        fe = FB.FbankFrontEnd(**cfg)
        sr = cfg.get("sample_rate", 16000)
        assert (fe.W, fe.S, fe.N) == R.geometry(sr, 25.0, 10.0)
        w, tw, bank, wt = fe.tables("cpu")
        assert w.dtype == torch.float32 and tw.dtype == torch.float64 and bank.dtype == torch.int32 and wt.dtype == torch.float32
        assert np.array_equal(w.numpy(), R.window(cfg.get("window_type", "povey"), fe.W).astype(np.float32))
        assert abs(w[0] - (0.08 if cfg.get("window_type") == "hamming" else 0.0)) < 1e-7 and (w - w.flip(0)).abs().max() < 1e-6, "symmetric, not periodic"
        k = np.arange(fe.N // 2)
        assert np.abs(tw.numpy() - np.concatenate([np.cos(2 * np.pi * k / fe.N), -np.sin(2 * np.pi * k / fe.N)])).max() < 1e-15
        dense = R.mel_bank(fe.num_mel_bins, fe.N, sr, cfg.get("low_freq", 20.0), cfg.get("high_freq", 0.0))
        back = np.zeros_like(dense)
        for j, (first, cnt, off) in enumerate(bank.tolist()):
            back[j, first:first + cnt] = wt.numpy()[off:off + cnt]
            assert (wt.numpy()[off:off + cnt] > 0).all() or cnt == 0
        assert np.abs(back - dense).max() < 1e-7
        assert bank[:, 1].sum() == len(wt) <= fe.N and (bank[:, 2] == torch.cumsum(bank[:, 1], 0) - bank[:, 1]).all()
        assert fe.tables("cpu") is fe.tables(torch.device("cpu")), "made once per device"
    assert FB.FbankFrontEnd(num_mel_bins=128, sample_rate=8000).tables("cpu")[2][:, 1].min() == 0, "a bin between two FFT bins is empty"


def test_configurations_outside_the_kernel_are_value_errors():
    for bad in (dict(sample_rate=44100), dict(sample_rate=4000), dict(frame_length=65.0), dict(num_mel_bins=0), dict(num_mel_bins=129),
                dict(window_type="blackman"), dict(preemphasis=1.5), dict(frame_shift=0.01), dict(low_freq=9000.0), dict(high_freq=9000.0)):
        with pytest.raises(ValueError, match="FbankFrontEnd"):
            FB.FbankFrontEnd(**bad)
    fe = FB.FbankFrontEnd()
    assert [fe.num_frames(n) for n in (0, 399, 400, 559, 560, 16000)] == [0, 0, 1, 1, 2, 98]
    assert FB.FbankFrontEnd(frame_length=R.ms_for(257, 16000)).N == 512 and FB.FbankFrontEnd(frame_length=R.ms_for(1024, 16000)).N == 1024


def _write(path, data, chans, width, rate=16000):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(chans)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(data.tobytes())


def test_read_wav(tmp_path):
    x = R.signal("noise3000", 1000, 3)
    _write(tmp_path / "mono.wav", x, 1, 2, 8000)
    got, rate = FB.read_wav(str(tmp_path / "mono.wav"))
    assert rate == 8000 and got.dtype == torch.int16 and np.array_equal(got.numpy(), x)
    _write(tmp_path / "stereo.wav", np.stack([x, -x], 1).astype("<i2"), 2, 2)
    got, rate = FB.read_wav(str(tmp_path / "stereo.wav"))
    assert rate == 16000 and np.array_equal(got.numpy(), x), "channel 0"
    _write(tmp_path / "eight.wav", (x // 256 + 128).astype(np.uint8), 1, 1)
    with pytest.raises(ValueError, match="8-bit"):
        FB.read_wav(str(tmp_path / "eight.wav"))
    (tmp_path / "junk.wav").write_bytes(b"not a wav file at all")
    with pytest.raises(ValueError, match="not a PCM wav"):
        FB.read_wav(str(tmp_path / "junk.wav"))
    _write(tmp_path / "empty.wav", x[:0], 1, 2)
    assert FB.read_wav(str(tmp_path / "empty.wav"))[0].numel() == 0


# ------------------------------------------------------------------ host logic on the numpy reference
@pytest.fixture
def calls(monkeypatch):
    c = []

    def fbank(waves, wave_len, window, twiddle, bank, weights, S, N, preemph=0.97, remove_dc=True):
        assert waves.dtype in (torch.int16, torch.float32) and wave_len.dtype == torch.int64
        c.append(("fbank", tuple(waves.shape), S, N, preemph, remove_dc))
        W, F = window.shape[0], bank.shape[0]
        B, Nmax = waves.shape
        out = torch.full((B, R.num_frames(Nmax, W, S), F), 7.0)
        out_len, status = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
        for b in range(B):
            n = int(wave_len[b])
            if not 0 <= n <= Nmax:
                status[b] = 2
                m = 0
            else:
                got = R.fbank(waves[b, :n].numpy(), sr={256: 8000, 512: 16000, 1024: 22050}[N], num_mel_bins=F, preemphasis=preemph,
                              remove_dc_offset=remove_dc)
                m = len(got)
                out[b, :m] = torch.from_numpy(got).float()
                status[b] = 0 if m else 1
            out_len[b] = m
            out[b, m:] = 0
        return out, out_len, status

    def cmvn(x, lengths):
        assert x.dtype == torch.float32 and x.is_contiguous() and lengths.dtype in (torch.int32, torch.int64)
        c.append(("cmvn", tuple(x.shape)))
        out_len, status = torch.zeros(len(x), dtype=torch.int32), torch.zeros(len(x), dtype=torch.int32)
        for b in range(len(x)):
            n = int(lengths[b])
            if not 0 <= n <= x.shape[1]:
                status[b], n = 2, 0
            elif n < 2:
                status[b], n = 1, 0
            else:
                x[b, :n] = torch.from_numpy(R.cmvn(x[b, :n].numpy()).astype(np.float32))
            out_len[b] = n
            x[b, n:] = 0
        return out_len, status
    monkeypatch.setattr(FB.K, "fbank", fbank)
    monkeypatch.setattr(FB.K, "cmvn", cmvn)
    return c


def _batch():
    x = torch.from_numpy(np.stack([R.signal("noise3000", 2000, s) for s in range(5)]))
    return x, torch.tensor([2000, 1000, 399, 400, 2001])


def test_features_without_normalisation(calls):
    x, n = _batch()
    fe = FB.FbankFrontEnd(normalize=False)
    out = fe.features(x, n)
    assert sorted(out) == ["features", "lengths", "status"] and calls == [("fbank", (5, 2000), 160, 512, 0.97, True)]
    assert out["features"].dtype == torch.float32 and tuple(out["features"].shape) == (5, 11, 80)
    assert out["lengths"].dtype == torch.int64 and out["lengths"].tolist() == [11, 4, 0, 1, 0] and out["status"].tolist() == [0, 0, 1, 0, 2]
    assert np.abs(out["features"][1, :4].numpy() - R.fbank(x[1, :1000].numpy())).max() < 1e-5 and out["features"][1, 4:].eq(0).all()
    ni = fe.net_input(x.float(), n.int())
    assert sorted(ni) == ["src_lengths", "src_tokens"] and torch.equal(ni["src_tokens"], out["features"]) and torch.equal(ni["src_lengths"], out["lengths"])
    assert calls[-1] == calls[0] and fe.features(x.double(), n.tolist())["lengths"].tolist() == [11, 4, 0, 1, 0]
    with pytest.raises(ValueError, match="int16 or floating"):
        fe.features(x.long(), n)
    with pytest.raises(ValueError, match="Nmax"):
        fe.features(x[0], n[:1])


def test_features_with_normalisation_merge_the_statuses(calls):
    x, n = _batch()
    fe = FB.FbankFrontEnd(preemphasis=0.9, remove_dc_offset=False)
    out = fe.features(x, n)
    assert calls == [("fbank", (5, 2000), 160, 512, 0.9, False), ("cmvn", (5, 11, 80))]
    assert out["lengths"].tolist() == [11, 4, 0, 0, 0] and out["status"].tolist() == [0, 0, 1, 1, 2], "one frame has no variance; a refusal stays one"
    want = R.cmvn(R.fbank(x[0].numpy(), preemphasis=0.9, remove_dc_offset=False).astype(np.float32))
    assert np.abs(out["features"][0].numpy() - want).max() < 1e-4 and out["features"][2:].eq(0).all()


def test_normalize_features_alone_works_on_a_copy(calls):
    fe = FB.FbankFrontEnd(num_mel_bins=40)
    x = torch.from_numpy(np.random.default_rng(0).normal(12, 2, (3, 9, 40))).double()
    keep = x.clone()
    out = fe.normalize_features(x, [9, 5, 12])
    assert calls == [("cmvn", (3, 9, 40))] and torch.equal(x, keep), "the argument is left alone"
    assert out["features"].dtype == torch.float32 and out["lengths"].tolist() == [9, 5, 0] and out["status"].tolist() == [0, 0, 2]
    assert np.abs(out["features"][1, :5].numpy() - R.cmvn(keep[1, :5].float().numpy())).max() < 1e-5 and out["features"][1, 5:].eq(0).all()
