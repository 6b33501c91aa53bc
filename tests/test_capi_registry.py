"""The build table busca_amd.build.LIBS and the bindings of the context-free libraries agree: every entry but libbusca_hip.so has a binding
busca_amd._<stem>_lib whose path, header and API table are the entry's, and whose load() and check() (busca_amd._capi.bind) work without a GPU."""
import importlib
import os

import pytest

from busca_amd import _lib
from busca_amd import build as builder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTEXT_FREE = [entry for entry in builder.LIBS if entry[0] != "hip"]


def test_the_table_names_the_eleven_libraries():
    stems = [stem for stem, _, _ in builder.LIBS]
    assert stems == ["track", "store", "rounds", "sort", "frame", "sframe", "mframe", "msframe", "gframe", "mgframe", "hip"]
    assert builder.OUT == builder.lib_path("hip") and (builder.UNITS, builder.HEADERS) == builder.LIBS[-1][1:]
    assert os.path.basename(builder.build()) == "libbusca_hip.so"


@pytest.mark.parametrize("stem,units,headers", CONTEXT_FREE, ids=[entry[0] for entry in CONTEXT_FREE])
def test_binding_matches_the_table(stem, units, headers):
    builder.build()
    mod = importlib.import_module("busca_amd._%s_lib" % stem)
    path = getattr(mod, stem.upper() + "_LIB_PATH")
    assert path == builder.lib_path(stem) == getattr(builder, stem.upper() + "_OUT") and os.path.exists(path)
    assert units == [("busca_%s" % stem, False)]
    assert mod.HEADER == headers[0] == "busca_%s.h" % stem and os.path.exists(os.path.join(ROOT, "include", mod.HEADER))
    api = getattr(mod, stem.upper() + "_API")
    assert all(name.startswith("busca_%s_" % stem) for name in api)
    assert {"busca_%s_version" % stem, "busca_%s_last_error" % stem} <= set(api)
    lib = mod.load()
    assert lib is mod.load() is mod._lib
    assert getattr(lib, "busca_%s_version" % stem)() // 1000 == mod.ABI_MAJOR
    assert mod.check(0) is None
    with pytest.raises(_lib.BuscaError, match="^libbusca_%s error -1: " % stem):
        mod.check(-1)
