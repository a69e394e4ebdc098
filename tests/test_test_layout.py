"""No GPU, no library: how the tests themselves are laid out.  A test module states what is expected and is nobody's library, so no
file under tests/ imports a tests.test_* module, at its top level or inside a function -- but for the two CPU tests named in JUDGED,
which load the GPU test module whose case list they hold to its promises: it is the thing they judge, not their library --; the
helper modules import on a machine without a GPU; and the three equality judges of
tests/stream_harness.py tell apart what their names promise."""
import glob
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import stream_harness as SH

HERE = os.path.dirname(os.path.abspath(__file__))
SIBLING = re.compile(r"^[ \t]*(from\s+tests\.test_\w+\s+import\b|from\s+tests\s+import\s+(\(\s*)?(\w+\s*,\s*)*test_\w+|import\s+tests\.test_\w+)", re.M)
# file: the one import of a test module it may contain (tests/test_logprob_kernels.py and tests/test_slot_forward_kernels.py build their
# case lists without a GPU so that these CPU tests can inspect them); nothing is to be added here
JUDGED = {"test_logprob_ref.py": "from tests import test_logprob_kernels", "test_slot_forward_ref.py": "from tests import test_slot_forward_kernels"}
F32 = np.float32


def test_no_test_module_is_imported_by_another_file():
    found = []
    for path in sorted(glob.glob(os.path.join(HERE, "**", "*.py"), recursive=True)):
        with open(path) as f:
            found += [(os.path.relpath(path, HERE), m.group(0).strip()) for m in SIBLING.finditer(f.read())]
    assert sorted(found) == sorted(JUDGED.items()), found


def test_the_pattern_sees_every_form_of_the_import():
    for line in ("from tests.test_a import b", "    from tests.test_a import b", "from tests import test_a", "from tests import x, test_a as K",
                 "\tfrom tests import test_a as K", "import tests.test_a", "        import tests.test_a as K", "x = 1\nfrom tests.test_a import b"):
        assert SIBLING.search(line), line
    for line in ("from tests.stream_harness import host", "from tests import score_ref as R", "# from tests.test_a import b", "x = 'tests.test_a'"):
        assert not SIBLING.search(line), line


@pytest.mark.parametrize("name", ["stream_harness", "stream_cases", "pass_cases", "kernel_unit", "abi_host"])
def test_the_helper_modules_import_without_a_gpu(name, monkeypatch):
    """The module's own top level, run again under another name with no device to be had and every way to one refusing."""
    def refuse(*a, **k):
        raise AssertionError("importing tests/{}.py touched the device".format(name))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(torch.cuda, "_lazy_init", refuse)
    spec = importlib.util.spec_from_file_location("layout_probe_" + name, os.path.join(HERE, name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    assert not torch.cuda.is_available() and module.__doc__


def _fails(judge, a, b, **kw):
    with pytest.raises(AssertionError):
        judge(a, b, **kw)
    return True


def test_same_bits_compares_float32_words_and_other_dtypes_by_value():
    zero, minus = dict(x=np.zeros(3, F32)), dict(x=-np.zeros(3, F32))
    assert _fails(SH.same_bits, zero, minus)
    nan = np.array([0x7fc00000, 0x7fc00001], np.uint32).view(F32)
    SH.same_bits(dict(x=nan[:1]), dict(x=nan[:1].copy()))
    assert _fails(SH.same_bits, dict(x=nan[:1]), dict(x=nan[1:]))
    SH.same_bits(dict(i=np.arange(3, dtype=np.int32)), dict(i=np.arange(3, dtype=np.int64)))      # other dtypes: by value
    SH.same_bits(dict(x=zero["x"], y=nan[:1]), dict(x=zero["x"], y=nan[1:]), ["x"])               # only the keys named
    with pytest.raises(AssertionError, match="step 3.*'x'"):
        SH.same_bits(zero, minus, where="step 3")


def test_same_values_takes_any_nan_for_any_nan_and_minus_zero_for_zero():
    SH.same_values(dict(x=np.zeros(3, F32)), dict(x=-np.zeros(3, F32)))
    nan = np.array([0x7fc00000, 0x7fc00001], np.uint32).view(F32)
    SH.same_values(dict(x=nan[:1]), dict(x=nan[1:]))
    assert _fails(SH.same_values, dict(x=np.zeros(3, F32)), dict(x=np.ones(3, F32)))


def test_same_bytes_holds_dtype_and_shape_too():
    one = np.ones((2, 3), F32)
    SH.same_bytes(dict(x=one, t=torch.ones(2)), dict(x=one.copy(), t=torch.ones(2)))
    assert _fails(SH.same_bytes, dict(x=one), dict(x=one.astype(np.float64)))
    assert _fails(SH.same_bytes, dict(x=one), dict(x=one.reshape(3, 2)))
    assert _fails(SH.same_bytes, dict(x=one), dict(x=one.reshape(1, 2, 3)))
    assert _fails(SH.same_bytes, dict(x=np.zeros(2, F32)), dict(x=-np.zeros(2, F32)))
    nan = np.array([0x7fc00000], np.uint32).view(F32)
    SH.same_bytes(dict(x=nan), dict(x=nan.copy()))


@pytest.mark.parametrize("judge", [SH.same_bits, SH.same_values, SH.same_bytes])
def test_the_recursive_forms_hold_the_key_sets(judge):
    a = dict(x=np.ones(2, F32), lane=dict(box=np.ones(2, F32), score=dict(tp=np.ones(1, np.int32))))
    same = dict(x=np.ones(2, F32), lane=dict(box=np.ones(2, F32), score=dict(tp=np.ones(1, np.int32))))
    judge(a, same)
    assert _fails(judge, a, dict(same, y=np.ones(1, F32)))
    assert _fails(judge, a, dict(same, lane=dict(box=np.ones(2, F32))))
    assert _fails(judge, a, dict(same, lane=dict(same["lane"], score=dict(tp=np.ones(1, np.int32), fn=np.ones(1, np.int32)))))
    assert _fails(judge, a, dict(same, lane=dict(same["lane"], score=dict(tp=np.zeros(1, np.int32)))))


def test_host_keeps_a_nested_dicts_structure():
    out = dict(what=torch.ones(2, 3), lane=dict(box=torch.zeros(2, 4), score=dict(tp=torch.ones(1, dtype=torch.int32))))
    got = SH.host(out)
    assert set(got) == {"what", "lane"} and set(got["lane"]) == {"box", "score"} and set(got["lane"]["score"]) == {"tp"}
    assert isinstance(got["what"], np.ndarray) and got["what"].shape == (2, 3) and got["lane"]["box"].dtype == F32
    assert got["lane"]["score"]["tp"].dtype == np.int32 and got["lane"]["score"]["tp"].tolist() == [1]
