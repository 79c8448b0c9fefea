"""The kernel-route options of s2t_set_option: the keys the library accepts (csrc/runtime.hip), the keys the header documents
(include/s2t_hip.h) and the keys tests/test_routes_gpu.py sets must stay the same set, so that "tests cover every route" stays true
when a route is added."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# keys that are not kernel routes: decode_stop_after is a diagnostic that truncates a decode step after that many launches
EXEMPT = {"decode_stop_after"}


def _read(*parts):
    with open(os.path.join(REPO, *parts)) as f:
        return f.read()


def library_keys():
    src = _read("fbk_fairseq_st_amd", "csrc", "runtime.hip")
    body = src[src.index('extern "C" int s2t_set_option'):]
    body = body[:body.index("nullptr;")]
    return set(re.findall(r'!strcmp\(key, "(\w+)"\)', body))


def header_keys():
    src = _read("include", "s2t_hip.h")
    start = src.index("---- kernel-route options")
    block = src[start:src.index("int s2t_set_option(", start)]
    return set(re.findall(r'"(\w+)"\s*(?:/\s*"(?:\w+)")?\s*(?:\(|:)', block)) | set(re.findall(r'/ "(\w+)"', block))


def test_option_parser_sees_exactly_the_known_keys():
    assert library_keys() == {"gemm256", "attn_v1", "attn_v2_min_tq", "gemm256_min_tiles", "decode_stop_after", "reserve_cus",
                              "gemm_f32_small_nt", "gemm_f32_small_kt", "gemm_f32_narrow", "gemm_small_nt", "gemm_small_kt",
                              "gemm_deep", "ln_small"}, library_keys()


def test_header_documents_exactly_the_library_keys():
    assert header_keys() == library_keys(), ("documented only", header_keys() - library_keys(),
                                             "accepted only", library_keys() - header_keys())


def test_every_route_key_is_set_by_the_route_tests():
    src = _read("tests", "test_routes_gpu.py")
    missing = {k for k in library_keys() - EXEMPT if not re.search(r'set_option\("%s"' % re.escape(k), src)}
    assert not missing, "route options no GPU test sets: %s" % sorted(missing)
