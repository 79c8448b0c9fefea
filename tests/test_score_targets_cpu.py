"""s2t_score_targets at the C-ABI boundary, without a GPU: the symbol is exported and bound, SequenceScorer imports, and every
argument check of include/s2t_hip.h answers before anything is launched -- through ctypes and through the generated binding alike
(the pattern of tests/test_abi_cpu.py::test_argument_validation_without_gpu)."""
import ctypes

import pytest

from fbk_fairseq_st_amd import lib as L

OK, EINVAL, ENOTSUP = 0, -22, -95
F32, BF16 = L.F32, L.BF16
X = 0x10000                       # stands for a device pointer: no call below gets as far as a launch


def _arrays(n, ptrs=None, lds=None, V=8):
    p = (ctypes.c_void_p * max(n, 1))(*(ptrs if ptrs is not None else [X] * n))
    l = (ctypes.c_int * max(n, 1))(*(lds if lds is not None else [V] * n))
    return p, l


def _cases():
    """(name, expected code, arguments after the two host arrays are filled in by the caller)"""
    V = 8
    c = []
    # B * L == 0 answers S2T_OK at once, whatever else is passed
    c.append(("B = 0", OK, dict(B=0, L=5)))
    c.append(("L = 0", OK, dict(B=3, L=0)))
    c.append(("B*L = 0 before every other check", OK, dict(B=0, L=0, n=0, target=0, out=0, V=0, dtype=7)))
    c.append(("n = 0", EINVAL, dict(n=0)))
    c.append(("n = -1", EINVAL, dict(n=-1)))
    c.append(("n = 9", EINVAL, dict(n=9)))
    c.append(("NULL pointer array", EINVAL, dict(null_ptrs=True)))
    c.append(("NULL stride array", EINVAL, dict(null_lds=True)))
    c.append(("NULL member", EINVAL, dict(n=3, ptrs=[X, 0, X])))
    c.append(("NULL last member", EINVAL, dict(n=8, ptrs=[X] * 7 + [0])))
    c.append(("NULL target", EINVAL, dict(target=0)))
    c.append(("NULL out", EINVAL, dict(out=0)))
    c.append(("V = 0", EINVAL, dict(V=0, lds=[8])))
    c.append(("V = -3", EINVAL, dict(V=-3, lds=[8])))
    c.append(("ld < V", EINVAL, dict(lds=[V - 1])))
    c.append(("second ld < V", EINVAL, dict(n=2, lds=[V, V - 1])))
    c.append(("dtype 2", ENOTSUP, dict(dtype=2)))
    c.append(("dtype -1", ENOTSUP, dict(dtype=-1)))
    return c


def _call(fn, dtype=BF16, n=1, ptrs=None, lds=None, target=X, out=X, B=2, L=3, V=8, null_ptrs=False, null_lds=False):
    p, l = _arrays(n if 0 < n <= 8 else 1, ptrs, lds, V=max(V, 1))
    return fn(dtype, n, 0 if null_ptrs else ctypes.addressof(p), 0 if null_lds else ctypes.addressof(l), target, out, B, L, V, 0)


def test_library_exports_and_binds_score_targets():
    lib = L.load()
    assert "s2t_score_targets" in L.SIGNATURES and len(L.SIGNATURES["s2t_score_targets"]) == 10
    assert hasattr(lib, "s2t_score_targets")
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "s2t_score_targets")
    assert lib.s2t_abi_version() == 9


def test_sequence_scorer_imports():
    from fbk_fairseq_st_amd import kernels, sequence_generator
    from fbk_fairseq_st_amd.sequence_scorer import SequenceScorer
    assert callable(kernels.score_targets) and callable(SequenceScorer.generate)
    assert callable(sequence_generator.hard_alignment)


@pytest.mark.parametrize("name,code,kw", _cases(), ids=[c[0] for c in _cases()])
def test_argument_checks_through_ctypes(name, code, kw):
    L.load()
    raw = L.load_ctypes()
    assert _call(raw.s2t_score_targets, **kw) == code, name


def test_argument_checks_through_the_generated_binding():
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None, "the generated binding did not load"
    assert hasattr(fast, "s2t_score_targets")
    for name, code, kw in _cases():
        assert _call(fast.s2t_score_targets, **kw) == code, name
    with pytest.raises(TypeError):
        fast.s2t_score_targets(0, 1)


def test_build_generator_refusal_names_the_class():
    """registry.build_generator keeps refusing --score-reference (tests/test_decode_diverse_cpu.py pins that) and says where to go"""
    from fbk_fairseq_st_amd.data import Dictionary
    from fbk_fairseq_st_amd.registry import FairseqTask, namespace

    class T(FairseqTask):
        def __init__(self, tgt):
            self._tgt = tgt

        @property
        def target_dictionary(self):
            return self._tgt
    with pytest.raises(NotImplementedError, match=r"sequence_scorer\.SequenceScorer"):
        T(Dictionary.synthetic(96)).build_generator([], namespace(beam=6, score_reference=True))
