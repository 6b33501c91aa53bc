"""The one loader of the context-free libraries libbusca_<stem>.so (busca_amd.build.LIBS, all but libbusca_hip.so): each binding _<stem>_lib.py keeps
its constants and its <STEM>_API table and takes its load() and check() from bind().  _lib.py loads libbusca_hip.so by its own rules (an override of
the path, several tables, errors that belong to a context).  No fallback: a missing library raises."""
import ctypes as C
import os
import sys

from ._lib import BuscaError

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path(stem):
    return os.path.join(_HERE, "libbusca_%s.so" % stem)


def bind(module, stem, api, abi_major):
    """-> (load, check) of the binding `module` (its __name__) of libbusca_<stem>.so.  `api`: name -> (restype, argtypes), the mirror of
    include/busca_<stem>.h; `abi_major`: busca_<stem>_version() // 1000 the binding was written for.  The loaded library is kept in the binding's
    own `_lib`."""
    path, so = lib_path(stem), "libbusca_%s" % stem

    def load():
        """dlopen the in-tree library and type every entry point.  Raises if it has not been built."""
        mod = sys.modules[module]
        if mod._lib is None:
            if not os.path.exists(path):
                raise ImportError("%s is missing - run `python -m busca_amd.build` (hipcc, gfx950). busca_amd has no CPU fallback." % path)
            import torch  # noqa: F401  (first, so that this library binds to the HIP runtime torch brought: see _lib.load)
            lib = C.CDLL(path)
            for name, (res, args) in api.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            v = getattr(lib, "busca_%s_version" % stem)()
            if v // 1000 != abi_major:
                raise ImportError("%s.so has ABI version %d, this binding needs major %d - rebuild (python -m busca_amd.build --force)" % (so, v, abi_major))
            mod._lib = lib
        return mod._lib

    def check(rc):
        """Raise BuscaError with the library's message for a non-zero return code."""
        if rc != 0:
            raise BuscaError("%s error %d: %s" % (so, rc, getattr(load(), "busca_%s_last_error" % stem)().decode()))

    return load, check
