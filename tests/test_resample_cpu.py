"""The resampler without a GPU: the entry point is exported, bound and refuses bad arguments before anything is launched, in the
order the header states; the limits are the same in the header, in kernels and in the module, and each is refused at its first value
outside and accepted at the last inside; the packed table is what the rule says; and the host logic of WaveResampler and SpeedPerturb
-- result keys, dtypes, Mmax, the draws, the table cache -- with kernels.resample replaced by the numpy reference
(tests/resample_ref.py; the kernel has its own tests)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import resample_ref as R
from fbk_fairseq_st_amd import kernels as K
from fbk_fairseq_st_amd import lib as L
from fbk_fairseq_st_amd import resample as RS

FAKE = 1 << 20            # a non-null pointer: a refused call reads and writes nothing


def host_banks(*rows):
    a = (ctypes.c_int * (7 * len(rows)))(*[v for r in rows for v in r])
    return a, ctypes.addressof(a)


GOOD = (3, 1, 37, 0, 0, -18, 37)          # 48 k -> 16 k
KEEP, GOOD_PTR = host_banks(GOOD)
ARGS = (("waves", FAKE), ("wave_elem", 2), ("row_stride", 1000), ("lengths", FAKE), ("len_elem", 8), ("ratio_id", None), ("B", 2), ("Nmax", 1000),
        ("Mmax", 334), ("banks", GOOD_PTR), ("n_banks", 1), ("first", FAKE), ("n_first", 1), ("weights", FAKE), ("n_weights", 37), ("out", FAKE),
        ("out_len", FAKE), ("status", FAKE), ("stream", None))


def test_exports_bindings_and_limits():
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    assert "s2t_resample" in L.SIGNATURES and hasattr(raw, "s2t_resample") and hasattr(lib, "s2t_resample") and "s2t_resample" not in L._SIZE_T_RESULT
    assert len(L.SIGNATURES["s2t_resample"]) == len(ARGS)
    assert lib.s2t_abi_version() == 9
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s2t_hip.h")) as f:
        text = f.read()
    for name in ("MAX_BANKS", "BANK_INTS", "REUSE", "TILE_ITEMS", "MAX_PHASES", "MAX_BANK", "MAX_SPAN"):
        assert "#define S2T_RESAMPLE_%s %d\n" % (name, getattr(K, "RESAMPLE_" + name)) in text, name
    assert (RS.MAX_BANKS, RS.MAX_PHASES, RS.MAX_BANK, RS.MAX_SPAN) == (K.RESAMPLE_MAX_BANKS, K.RESAMPLE_MAX_PHASES, K.RESAMPLE_MAX_BANK, K.RESAMPLE_MAX_SPAN)
    assert K.RESAMPLE_MAX_BANK >= 5440 and K.RESAMPLE_TILE_ITEMS >= K.RESAMPLE_MAX_PHASES
    # what one workgroup stages is at most 64 KiB of LDS
    assert 4 * (K.RESAMPLE_MAX_BANK + K.RESAMPLE_MAX_PHASES + K.RESAMPLE_MAX_SPAN + 4) <= 65536
    import fbk_fairseq_st_amd
    assert not hasattr(fbk_fairseq_st_amd, "WaveResampler"), "the module is imported by its name"


def check_refusals(fn):
    f = lambda **kw: fn(*[kw.get(k, d) for k, d in ARGS])
    for name in ("waves", "lengths", "banks", "first", "weights", "out", "out_len", "status"):
        assert f(**{name: None}) == -22, name
    for bad in (dict(wave_elem=1), dict(wave_elem=8), dict(len_elem=2), dict(len_elem=0), dict(Nmax=-1), dict(Mmax=-1), dict(row_stride=-1),
                dict(n_first=-1), dict(n_weights=-1), dict(n_banks=0)):
        assert f(**bad) == -22, bad
    assert f(n_banks=9) == -95 and f(n_banks=9, wave_elem=3) == -22

    def one(row, **kw):
        keep, ptr = host_banks(row)
        return f(banks=ptr, **kw)
    for row in ((0, 1, 37, 0, 0, -18, 37), (3, 0, 37, 0, 0, -18, 37), (3, 1, 0, 0, 0, -18, 37), (3, 1, 37, 0, 0, -18, 36), (3, 1, 37, -1, 0, -18, 37),
                (3, 1, 37, 0, -1, -18, 37), (3, 1, 37, 1, 0, -18, 37), (3, 1, 37, 0, 1, -18, 37), (3, 1, 38, 0, 0, -18, 38), (3, 1, 37, 0, 0, -(1 << 30), 37)):
        assert one(row) == -22, row
    big = dict(n_first=1 << 20, n_weights=1 << 20)
    # each limit at its first refused value
    assert one((3, 513, 2, 0, 0, -1, 4), **big) == -95                       # S2T_RESAMPLE_MAX_PHASES
    assert one((1, 3, 2731, 0, 0, -1, 2731), **big) == -95                   # 8,193 weights: S2T_RESAMPLE_MAX_BANK
    assert one((3, 1, 37, 0, 0, -18, K.RESAMPLE_MAX_SPAN - 9 + 1), **big) == -95   # three units and the rest: S2T_RESAMPLE_MAX_SPAN
    assert one((2546, 1, 37, 0, 0, -18, 37), **big) == -95                   # 3 * 2546 + 37 = 7,675: in_unit
    # an invalid argument in a later bank is named before an unsupported one in an earlier bank
    keep, ptr = host_banks((3, 513, 2, 0, 0, -1, 4), (0, 1, 37, 0, 0, -18, 37))
    assert f(banks=ptr, n_banks=2, **big) == -22
    keep, ptr = host_banks(GOOD, (3, 513, 2, 0, 0, -1, 4))
    assert f(banks=ptr, n_banks=2, **big) == -95
    assert f(B=0) == 0 and f(B=-3) == 0 and f(B=0, waves=None, banks=None, n_banks=99) == 0       # an empty problem: nothing is looked at


def test_refusals_before_any_launch_and_their_order():
    check_refusals(L.load().s2t_resample)


def test_generated_binding_answers_like_ctypes():
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None
    raw = ctypes.CDLL(L.LIB_PATH)
    raw.s2t_resample.argtypes = L.SIGNATURES["s2t_resample"]
    check_refusals(fast.s2t_resample)
    check_refusals(raw.s2t_resample)


def banks_t(*rows):
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 7)


def test_each_limit_at_its_last_accepted_and_first_refused_value():
    ok = lambda row, nf=1 << 20, nw=1 << 20: K.resample_check_banks(banks_t(row), nf, nw)

    def refused(row, match, nf=1 << 20, nw=1 << 20):
        with pytest.raises(ValueError, match=match):
            K.resample_check_banks(banks_t(row), nf, nw)
    ok((3, 512, 2, 0, 0, -1, 4))
    refused((3, 513, 2, 0, 0, -1, 4), "S2T_RESAMPLE_MAX_PHASES")
    ok((1, 4, 2048, 0, 0, -1, 2048))                                        # 8,192 weights
    refused((1, 3, 2731, 0, 0, -1, 2731), "S2T_RESAMPLE_MAX_BANK")          # 8,193
    ok((3, 1, 37, 0, 0, -18, K.RESAMPLE_MAX_SPAN - 9))
    refused((3, 1, 37, 0, 0, -18, K.RESAMPLE_MAX_SPAN - 8), "S2T_RESAMPLE_MAX_SPAN")
    ok((2545, 1, 37, 0, 0, -18, 37))                                        # 3 * 2545 + 37 = 7,672
    refused((2546, 1, 37, 0, 0, -18, 37), "S2T_RESAMPLE_MAX_SPAN")
    ok((48000, 48000, 0, 0, 0, 0, 0))                                       # a copy: nothing else is looked at
    K.resample_check_banks(banks_t(*[GOOD] * 8), 1, 37)
    with pytest.raises(ValueError, match="S2T_RESAMPLE_MAX_BANKS"):
        K.resample_check_banks(banks_t(*[GOOD] * 9), 1, 37)
    for row in ((0, 1, 37, 0, 0, -18, 37), (3, 1, 0, 0, 0, -18, 37), (3, 1, 37, 0, 0, -18, 36)):
        refused(row, "resample")
    refused(GOOD, "resample", nw=36)
    refused(GOOD, "resample", nf=0)
    for bad in (banks_t(GOOD).long(), banks_t(GOOD)[:, :6], banks_t(GOOD)[:0], banks_t(GOOD)[0]):
        with pytest.raises(ValueError, match="banks"):
            K.resample_check_banks(bad, 1, 37)
    # the tile: the group count follows both limits
    assert K.resample_group(3, 1, 37) == 512 and K.resample_tile(3, 1, 37) == 2048
    assert K.resample_group(441, 160, 474) == 3 and K.resample_tile(441, 160, 474) == 1920
    assert K.resample_group(6, 1, 73) == 316 and K.resample_group(2546, 1, 37) == 0 and K.resample_tile(5, 5, 0) == 2048


def test_pairs_inside_and_outside_the_limits():
    for pair in R.PAIRS + [(3, 1), (2, 1), (1, 2), (441, 320), (160, 147), (6, 1), (48000, 8000), (1, 6)]:
        banks, first, weights = RS.WaveResampler(*pair).tables("cpu")
        iu, ou, taps, f_off, w_off, lo, extra = banks[0].tolist()
        assert (iu, ou) == R.reduce_pair(*pair) and K.resample_group(iu, ou, extra) >= 1
    with pytest.raises(ValueError, match="S2T_RESAMPLE_MAX_PHASES"):
        RS.WaveResampler(16000, 15999)
    with pytest.raises(ValueError, match="S2T_RESAMPLE_MAX_BANK"):
        RS.make_bank(1000, 499)
    with pytest.raises(ValueError, match="S2T_RESAMPLE_MAX_SPAN"):
        RS.WaveResampler(600, 1)
    for bad in (dict(orig_freq=0), dict(orig_freq=-16000), dict(new_freq=0), dict(orig_freq=44100.5), dict(new_freq="16000"), dict(orig_freq=True),
                dict(lowpass_filter_width=0), dict(lowpass_filter_width=2.5), dict(rolloff=0.0), dict(rolloff=1.5)):
        with pytest.raises(ValueError, match="resample"):
            RS.WaveResampler(**dict(dict(orig_freq=48000, new_freq=16000), **bad))
    assert RS.WaveResampler(48000.0, 16000).bank["in_unit"] == 3, "an integral float is a rate"


def test_the_packed_table_is_what_the_rule_says():
    sp = RS.SpeedPerturb(("9/10", 1, "11/10", "441/160"))
    banks, first, weights = sp.tables("cpu")
    assert banks.dtype == torch.int32 and first.dtype == torch.int32 and weights.dtype == torch.float32 and not banks.is_cuda
    assert tuple(banks.shape) == (4, 7) and banks[1].tolist() == [1, 1, 0, 0, 0, 0, 0]
    f_off = w_off = 0
    for r, pair in ((0, (9, 10)), (2, (11, 10)), (3, (441, 160))):
        in_unit, out_unit, f, count, w = R.bank(*pair)
        taps = w.shape[1]
        assert banks[r].tolist() == [in_unit, out_unit, taps, f_off, w_off, int(f.min()), int(f.max() - f.min()) + taps]
        assert np.array_equal(first[f_off:f_off + out_unit].numpy(), f)
        got = weights[w_off:w_off + taps * out_unit].numpy().reshape(taps, out_unit)          # tap-major
        assert np.array_equal(got, w.T.astype(np.float32))
        f_off, w_off = f_off + out_unit, w_off + taps * out_unit
    assert (f_off, w_off) == (first.shape[0], weights.shape[0])
    assert sp.tables("cpu") is sp.tables(torch.device("cpu")), "made once per device"
    rs = RS.WaveResampler(48000, 16000)
    assert rs.tables("cpu") is rs.tables("cpu") and rs.tables("cpu")[0].tolist() == [list(GOOD)]
    assert RS.WaveResampler(16000, 16000).tables("cpu")[0].tolist() == [[1, 1, 0, 0, 0, 0, 0]]


def test_kernels_check_their_operands():
    banks, first, weights = RS.WaveResampler(48000, 16000).tables("cpu")
    x, n = torch.zeros(2, 1000, dtype=torch.int16), torch.tensor([1000, 500])
    rid = torch.zeros(2, dtype=torch.int32)
    call = lambda *a, **kw: K.resample(*a, **dict(dict(Mmax=334), **kw))
    for bad in (lambda: call(x[0], n, banks, first, weights), lambda: call(x.long(), n, banks, first, weights), lambda: call(x, n.float(), banks, first, weights),
                lambda: call(x, n[:1], banks, first, weights), lambda: call(x, n, banks.long(), first, weights), lambda: call(x, n, banks, first.long(), weights),
                lambda: call(x, n, banks, first, weights.double()), lambda: call(x, n, banks, first, weights[:36]), lambda: call(x, n, banks, first[:0], weights),
                lambda: call(x, n, banks, first, weights, ratio_id=rid.long()), lambda: call(x, n, banks, first, weights, ratio_id=rid[:1]),
                lambda: call(x, n, banks, first, weights, Mmax=-1), lambda: call(x, n, banks, first, weights, Mmax=1 << 31)):
        with pytest.raises(ValueError, match="resample"):
            bad()
    out, out_len, status = call(x[:0], n[:0], banks, first, weights)                 # no rows: nothing is launched
    assert tuple(out.shape) == (0, 334) and out.dtype == torch.float32 and out_len.dtype == torch.int64 and status.dtype == torch.int32
    with pytest.raises(L.S2THipError, match="device tensors"):
        call(x, n, banks, first, weights)                                             # a host tensor never reaches a kernel


# ------------------------------------------------------------------ host logic on the numpy reference
@pytest.fixture
def calls(monkeypatch):
    c = []

    def resample(waves, wave_len, banks, first, weights, Mmax, ratio_id=None):
        assert waves.dtype in (torch.int16, torch.float32) and wave_len.dtype in (torch.int32, torch.int64)
        assert ratio_id is None or ratio_id.dtype == torch.int32
        c.append((tuple(waves.shape), Mmax, None if ratio_id is None else ratio_id.tolist()))
        B, Nmax = waves.shape
        out = torch.full((B, Mmax), 7.0)
        out_len, status = torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int32)
        for b in range(B):
            n, r = int(wave_len[b]), 0 if ratio_id is None else int(ratio_id[b])
            m = 0
            if not 0 <= n <= Nmax or not 0 <= r < len(banks):
                status[b] = 2
            else:
                y, _ = R.resample(waves[b].numpy(), n, int(banks[r, 0]), int(banks[r, 1]), dtype=np.float32)
                if len(y) > Mmax:
                    status[b] = 2
                else:
                    m = len(y)
                    out[b, :m] = torch.from_numpy(y)
                    status[b] = 0 if m else 1
            out_len[b] = m
            out[b, m:] = 0
        return out, out_len, status
    monkeypatch.setattr(RS.K, "resample", resample)
    return c


def _batch():
    rng = np.random.default_rng(3)
    return torch.from_numpy(rng.integers(-3000, 3000, (4, 900)).astype(np.int16)), torch.tensor([900, 451, 0, 901])


def test_wave_resampler_host_logic(calls):
    x, n = _batch()
    rs = RS.WaveResampler(48000, 16000)
    assert [rs.num_samples(v) for v in (4800, 4801, 1, 0, 900)] == [1600, 1601, 1, 0, 300]
    assert RS.num_samples(900, 44100, 16000) == 327 and RS.WaveResampler(8000, 16000).num_samples(900) == 1800
    out = rs.resample(x, n)
    assert sorted(out) == ["lengths", "status", "waves"] and calls == [((4, 900), 300, None)], "Mmax from the padded width, on the host"
    assert out["waves"].dtype == torch.float32 and tuple(out["waves"].shape) == (4, 300)
    assert out["lengths"].dtype == torch.int64 and out["lengths"].tolist() == [300, 151, 0, 0] and out["status"].tolist() == [0, 0, 1, 2]
    assert rs.resample(x.double(), n.tolist())["lengths"].tolist() == [300, 151, 0, 0] and rs.resample(x.float(), n.int())["status"].tolist() == [0, 0, 1, 2]
    with pytest.raises(ValueError, match="int16 or floating"):
        rs.resample(x.long(), n)
    with pytest.raises(ValueError, match="Nmax"):
        rs.resample(x[0], n[:1])


def test_speed_perturb_host_logic(calls):
    x, n = _batch()
    sp = RS.SpeedPerturb()
    assert sp.pairs == ((9, 10), (1, 1), (11, 10)) and sp.num_samples(900) == 1000 and sp.num_samples(900, 2) == 819 and sp.num_samples(900, 1) == 900
    out = sp.apply(x, n, update=7, choice=[0, 1, 2, 3])
    assert sorted(out) == ["choice", "lengths", "status", "waves"] and calls == [((4, 900), 1000, [0, 1, 2, 3])], "Mmax from the slowest factor"
    assert out["choice"].dtype == torch.int32 and out["lengths"].tolist() == [1000, 451, 0, 0] and out["status"].tolist() == [0, 0, 1, 2]
    assert torch.equal(out["waves"][1, :451], x[1, :451].float()) and out["waves"][1, 451:].eq(0).all()
    # the draws: the same for the same (seed, update), different across updates and seeds, every factor drawn
    a, b = sp.draw(64, 7), sp.draw(64, 7)
    assert a.dtype == torch.int32 and torch.equal(a, b) and torch.equal(a, RS.SpeedPerturb(seed=1).draw(64, 7))
    assert not torch.equal(a, sp.draw(64, 8)) and not torch.equal(a, RS.SpeedPerturb(seed=2).draw(64, 7))
    assert sorted(set(a.tolist())) == [0, 1, 2]
    drawn = sp.apply(x, n, update=7)
    assert drawn["choice"].tolist() == sp.draw(4, 7).tolist() == calls[-1][2]
    assert RS.SpeedPerturb((1.1, "0.9", 2)).pairs == ((11, 10), (9, 10), (2, 1))


def test_unparsable_factors_are_value_errors():
    for bad in (("fast",), ("1/0",), (0,), (-1,), ("-9/10",), (float("nan"),), (float("inf"),), (None,), (True,), (), tuple([1] * 9)):
        with pytest.raises(ValueError, match="SpeedPerturb"):
            RS.SpeedPerturb(bad)
    with pytest.raises(ValueError, match="S2T_RESAMPLE_MAX_PHASES"):
        RS.SpeedPerturb(("16000/15999",))
