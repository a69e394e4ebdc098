"""The harness of the host-side ABI tests (tests/test_*_host.py) and of the lane kernels' GPU tests: the header as text and as
sqair_amd/_abi.py parses it, a C compiler on programs that include it, handles that close themselves, the dummy structs the
refusal tests hand over, and the handles the lane solves' GPU tests keep.  Importable without a GPU and without a built library:
only lib() behind open_handle() loads one.

What a test expects -- a field list, a prototype, a phrase, a refusal's text -- stays with the test and is stated there in full; what
is here is how it obtains the thing it judges."""
import contextlib
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

from sqair_amd import _abi, _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = C.c_void_p(0x1000)     # a fake device address, never dereferenced: the calls it goes to are refused first
BIG = 1 << 50
LIBS = [None, _capi.WIDE_LIB_PATH]


# ------------------------------------------------------------------------------------------------ the header
@functools.lru_cache(maxsize=None)
def raw():
    """include/sqair_hip.h as it is written, read once."""
    with open(_abi.HEADER_PATH) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def code():
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/", "", raw(), flags=re.S)


def paragraph(first_words=None, until=None):
    """The header's text from `first_words` up to `until` (the whole of it by default) with the comments' line breaks unwrapped."""
    text = raw()
    start = 0 if first_words is None else text.index(first_words)
    return re.sub(r"\s*\n \*\s*", " ", text[start:len(text) if until is None else text.index(until, start)])


def phrases(doc, words):
    for word in words:
        assert word in doc, word


def stated_once(first_words):
    assert raw().count(first_words) == 1, first_words


def fields(struct):
    """[(type as C spells it, name)] of every field of a struct of the header, in order."""
    return [(_abi.spell(f) + ("[{}]".format(f.array_len) if f.array_len else ""), f.name) for f in _abi.header().structs[struct]]


def functions():
    return list(_abi.header().functions)


def prototype(name):
    """A function's declaration as one string: ``int sqair_set_score(SqairHandle* h, const SqairLaneScore* score, int T, int B)``."""
    ret, params = _abi.header().functions[name]
    return "{} {}({})".format(_abi.spell(ret), name, ", ".join(_abi.spell(p) + " " + p.name for p in params) or "void")


def constant(name):
    return _abi.header().constants[name]


# ------------------------------------------------------------------------------------------------ the compiler
def compiler():
    """The gcc command line up to the header's include path."""
    gcc_path = shutil.which("gcc")
    assert gcc_path, "gcc is part of the image"
    return [gcc_path, "-I" + os.path.join(ROOT, "include")]


def gcc(tmp_path, name, lines, run=True):
    """Compiles (and runs) a generated C file against the header; returns what it printed, or the compiler's exit status."""
    src = tmp_path / (name + ".c")
    src.write_text("\n".join(lines) + "\n")
    cmd = compiler() + ["-std=gnu11", str(src)]
    if not run:
        return subprocess.run(cmd + ["-fsyntax-only"], capture_output=True, text=True).returncode
    subprocess.check_call(cmd + ["-o", str(tmp_path / name)])
    return subprocess.run([str(tmp_path / name)], capture_output=True, text=True, check=True).stdout


def c_layout(tmp_path, structs):
    """What the compiler gives the header's structs: {struct: (sizeof, [offsetof of each field asked for])} of {struct: fields}."""
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "sqair_hip.h"', "int main(void) {"]
    for name, names in structs.items():
        lines.append('  printf("{0} %zu{1}\\n", sizeof({0}){2});'.format(name, " %zu" * len(names),
                                                                       "".join(", offsetof({}, {})".format(name, n) for n in names)))
    got = [l.split() for l in gcc(tmp_path, "c_layout", lines + ["  return 0;", "}"]).splitlines()]
    return {l[0]: (int(l[1]), [int(v) for v in l[2:]]) for l in got}


# ------------------------------------------------------------------------------------------------ handles
def open_handle(path=None, hw=(50, 50), **flags):
    """(lib, h): a handle of the library at `path` (the product build by default) for make_flags(**flags) on frames of hw."""
    lib = _capi.lib(path)
    cfg = make_config(make_flags(**flags), hw)
    h = C.c_void_p()
    assert lib.sqair_create(C.byref(cfg), C.byref(h)) == 0
    return lib, h


@contextlib.contextmanager
def handle(path=None, hw=(50, 50), **flags):
    """``with handle(...) as (lib, h)``: open_handle, destroyed on the way out."""
    lib, h = open_handle(path, hw, **flags)
    try:
        yield lib, h
    finally:
        lib.sqair_destroy(h)


def err(lib, h):
    return lib.sqair_last_error(h).decode()


def set_state(lib, h, B, state_in=DUMMY, state_out=DUMMY, src=DUMMY):
    assert lib.sqair_set_state(h, state_in, state_out, src, lib.sqair_state_bytes(h, B), B) == 0


def fwd_args(h, B, T=1, bind=("log_weights_per_timestep",), t_offset=0, obs=DUMMY):
    """The arguments of sqair_forward and its kin on dummy pointers, the outputs named in `bind` bound."""
    out = _capi.SqairOutputs(**{k: DUMMY.value for k in bind})
    return (h, DUMMY, DUMMY, obs, DUMMY, T, B, t_offset, C.byref(out), DUMMY, BIG, DUMMY)


# ------------------------------------------------------------------------------------------------ dummy structs
def dummy(struct_class, base, names, without=(), **scalars):
    """A struct whose pointer fields `names` hold distinct fake addresses by position (base + 0x100 * i), but for those in `without`."""
    return struct_class(**scalars, **{n: base + 0x100 * i for i, n in enumerate(names) if n not in without})


def estimate(iou_min=0.5, log_w=0x2000, best_row=0x3000, fields=(), without=(), **more):
    """A SqairLaneEstimate with best_row (and log_w) and the optional outputs named in `fields`."""
    return dummy(_capi.SqairLaneEstimate, 0x4000, fields, without, iou_min=iou_min, log_w=log_w, best_row=best_row, **more)


def score(iou_min=0.5, G=4, without=(), outputs=_capi.SCORE_FIELDS):
    """A SqairLaneScore with its inputs and the per-frame outputs named."""
    sc = dummy(_capi.SqairLaneScore, 0x5000, _capi.SCORE_INPUTS, without, iou_min=iou_min, G=G)
    for i, n in enumerate(outputs):
        setattr(sc, n, 0x7000 + 0x100 * i)
    return sc


def smc(ess_frac=0.5, seed=7, log_w=DUMMY.value, src_rows=DUMMY.value, **more):
    """A SqairSmc that draws its own uniforms: every out buffer a dummy, src_rows the map set_state registers."""
    f = dict(uniforms=None, log_z=DUMMY.value, log_evidence=DUMMY.value, ess=DUMMY.value, u_out=None, resampled=DUMMY.value)
    f.update(more)
    return _capi.SqairSmc(ess_frac=ess_frac, seed=seed, log_w=log_w, src_rows=src_rows, **f)


CARRY_B = 4
OTHER = C.c_void_p(0x2000)      # a second fake device address
train_smc = functools.partial(smc, ess_frac=1.0)      # (training resamples at every frame)


def carry(lib, h, smc=None, **kw):
    """A SqairCarry of CARRY_B lanes on dummy pointers, its state_bytes the handle's; ``smc``: the SqairSmc it points to."""
    f = dict(state_in=DUMMY.value, state_out=DUMMY.value, src_rows=DUMMY.value, state_bytes=lib.sqair_state_bytes(h, CARRY_B), B=CARRY_B)
    f.update(kw)
    c = _capi.SqairCarry(**f)
    if smc is not None:
        c.smc = C.pointer(smc)
    return c


# ------------------------------------------------------------------------------------------------ handles kept for a session
LANE_LIBS = {"product": None, "wide": _capi.WIDE_LIB_PATH}
_kept = {}


def kept_handle(key, path=None, hw=(50, 50), **flags):
    """open_handle once per key, kept for the session: the lane solves' GPU tests (tests/idf_cases.py, tests/hota_cases.py) open one
    handle per library."""
    if key not in _kept:
        _kept[key] = open_handle(path, hw, **flags)
    return _kept[key]
