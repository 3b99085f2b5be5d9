"""The cross-view prediction entry points through every layer: declared in include/mvhdp.h with their argument struct, listed in
ABI_SYMBOLS with ctypes signatures, exported by the library, wrapped by NativeSampler and NativeGroup, and named in the documents.  No GPU."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mvhdp_predict_items", "mvhdp_score_items")


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_header_declares_both_calls_and_the_struct():
    hdr = read("include", "mvhdp.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*mvhdp_handle\s+h\s*,\s*const\s+mvhdp_predict_args\s*\*" % n, code), n
    st = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*mvhdp_predict_args\s*;", code)
    assert st and [f.split()[-1].lstrip("*") for f in st.group(1).split(";") if f.strip()] == ["m", "exclude_present", "view_weights", "theta"]
    # the definition is the header's: the chain, the order, the excluded set, and that the mix is not applied
    for phrase in ("fma(theta_d[k], phi[w][k], s)", "equal scores by ascending type id", "Excluded set", "xview_ref.c"):
        assert phrase in hdr, phrase
    mix = hdr[hdr.index("useVectorsLambda: the sweep with"):hdr.index("int mvhdp_set_vectors_mix")]
    assert "mvhdp_predict_items" in mix and "mvhdp_score_items" in mix


def test_listed_and_typed_in_the_loader_and_exported_by_the_library():
    from mvtopicmodel_amd import _lib
    for n in NAMES:
        assert n in _lib.ABI_SYMBOLS
    assert [f[0] for f in _lib.PredictArgsC._fields_] == ["m", "exclude_present", "view_weights", "theta"]
    assert C.sizeof(_lib.PredictArgsC) == 24
    L = _lib.load_library()
    assert len(L.mvhdp_predict_items.argtypes) == 8 and len(L.mvhdp_score_items.argtypes) == 9
    assert L.mvhdp_predict_items.restype is C.c_int and L.mvhdp_score_items.restype is C.c_int
    assert L.mvhdp_predict_items(None, None, 0, 0, 1, None, None, None) == -1      # a NULL handle: MVHDP_ERR_INVALID_ARG, no device touched
    assert L.mvhdp_score_items(None, None, 0, 0, 0, None, None, None, None) == -1


def test_wrapped_for_both_classes_with_the_result_object():
    from mvtopicmodel_amd import native
    for cls in (native.NativeSampler, native.NativeGroup):
        assert list(inspect.signature(cls.predict_items).parameters) == ["self", "m", "view_weights", "n", "d0", "d1", "exclude_present", "theta"]
        assert list(inspect.signature(cls.score_items).parameters) == ["self", "m", "view_weights", "entities", "items", "d0", "d1", "exclude_present", "theta"]
        assert inspect.signature(cls.predict_items).parameters["exclude_present"].default is True
    import numpy as np
    r = native.ItemScores(np.array([0.5, 0.25, 0.125, 1.0]), np.array([0, 1, 3, 9], dtype=np.int32))
    assert r.mean_log_score() == float(np.mean(np.log([0.5, 0.25, 0.125, 1.0]))) and r.recall_at(1) == 0.25 and r.recall_at(4) == 0.75
    assert r.mrr() == (1 + 0.5 + 0.25 + 0.1) / 4


def test_the_source_is_built_and_the_documents_name_the_calls():
    assert "mvhdp_xview.hip" in re.search(r"^SRCS\s*=(.*)$", read("mvtopicmodel_amd", "csrc", "Makefile"), flags=re.M).group(1)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "CHANGELOG.md"):
        text = read(doc)
        for n in NAMES:
            assert n in text, (doc, n)
    integ = read("INTEGRATION.md")
    assert "view_weights[m] = 0" in integ
