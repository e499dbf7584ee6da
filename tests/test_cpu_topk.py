"""Host-side checks of top-K retrieval (csrc/topk.hip, clipmi.evaluation.topk) that need no GPU: the version,
the header and the exports, argument validation of clipmi_topk_merge before any HIP call, and the ValueErrors of
the Python entry point."""
import os
import re

import pytest
import torch

from test_cpu_eval import BLOCK_CASES, PTR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPK_MAX = 256
ARGS = ("S", "lds", "N", "M", "row0", "rows", "col0", "cols", "k", "first", "exclude", "top_score", "top_idx")
# the block geometry of tests/test_cpu_eval.py: its target / target_score cases are not arguments here
GEOMETRY_CASES = [kw for kw in BLOCK_CASES if set(kw) <= set(ARGS)]


def _lib():
    from clipmi import _lib as L
    from clipmi import evaluation  # noqa: F401  (declares the prototypes)
    return L


def _merge(L, **kw):
    a = dict(S=PTR, lds=128, N=300, M=400, row0=128, rows=128, col0=256, cols=128, k=10, first=1, exclude=PTR,
             top_score=PTR, top_idx=PTR)
    a.update(kw)
    return L.lib().clipmi_topk_merge(None, *(a[n] for n in ARGS))


def test_version_is_at_least_4():
    assert _lib().lib().clipmi_version() >= 4


def test_header_declares_and_library_exports_topk_merge():
    with open(os.path.join(REPO, "include", "clipmi.h"), encoding="utf-8") as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+clipmi_topk_merge\s*\(", src)
    m = re.search(r"#define\s+CLIPMI_TOPK_MAX\s+(\d+)", src)
    assert m and int(m.group(1)) == TOPK_MAX
    assert hasattr(_lib().lib(), "clipmi_topk_merge")


def test_names_resolve_from_the_package():
    import clipmi
    from clipmi import evaluation
    for name in ("TopK", "topk"):
        assert getattr(clipmi, name) is getattr(evaluation, name)
    assert evaluation.TOPK_MAX == TOPK_MAX


def test_geometry_cases_cover_the_block():
    assert len(GEOMETRY_CASES) == len(BLOCK_CASES) - 2
    assert {k for kw in GEOMETRY_CASES for k in kw} == {"N", "M", "rows", "cols", "lds", "row0", "col0", "S"}


@pytest.mark.parametrize("kw", GEOMETRY_CASES + [dict(k=0), dict(k=-1), dict(k=TOPK_MAX + 1), dict(top_score=None),
                                                 dict(top_idx=None)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_topk_merge_rejects_bad_arguments_without_gpu(kw):
    L = _lib()
    st = _merge(L, **kw)
    assert st == -1 and b"clipmi_topk_merge" in L.lib().clipmi_last_error()
    with pytest.raises(ValueError):
        L.check(st, "clipmi_topk_merge")


def test_topk_merge_messages_name_the_fault():
    L = _lib()
    assert _merge(L, lds=100) == -1 and b"leading dimension" in L.lib().clipmi_last_error()
    assert _merge(L, k=TOPK_MAX + 1) == -1 and b"CLIPMI_TOPK_MAX" in L.lib().clipmi_last_error()
    assert _merge(L, top_idx=None) == -1 and b"null output" in L.lib().clipmi_last_error()


def test_topk_raises_value_error_on_bad_arguments():
    from clipmi.evaluation import topk
    q, c = torch.zeros(5, 8), torch.zeros(7, 8)
    with pytest.raises(ValueError, match="GPU tensors"):
        topk(q, c, 3)  # CPU tensors: no fallback
    with pytest.raises(ValueError, match=r"\[N, E\]"):
        topk(q, torch.zeros(7, 9), 3)  # mismatched E
    with pytest.raises(ValueError, match=r"\[N, E\]"):
        topk(q[0], c, 3)
    # (an empty input is told apart from a CPU tensor only on the GPU: tests/test_gpu_topk.py)
    with pytest.raises(ValueError):
        topk(torch.zeros(0, 8), c, 3)
    for k in (0, -1, TOPK_MAX + 1):
        with pytest.raises(ValueError, match="k must be"):
            topk(q, c, k)
    with pytest.raises(ValueError, match="exclude"):
        topk(q, c, 3, exclude=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="exclude"):
        topk(q, c, 3, exclude=torch.zeros(5, 1, dtype=torch.int64))
