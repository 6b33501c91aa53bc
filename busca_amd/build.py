"""Build the libraries of LIBS below - libbusca_hip.so and the context-free libbusca_<stem>.so - in-tree with hipcc for gfx950 (cross-compiles without
a GPU).

A library is one or several translation units (csrc/busca_internal.hpp lists those of libbusca_hip.so) compiled IN PARALLEL into busca_amd/build/*.o
and linked: a full build is as long as its slowest unit, and an edit recompiles only the units that include the edited file."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
VGPR_FORM = ["-mllvm", "-amdgpu-mfma-vgpr-form"]
# (stem, units, headers) of libbusca_<stem>.so, in build order.  A unit is (name, compiled with -amdgpu-mfma-vgpr-form where that compiles); the first
# header is the library's own under include/.  Each library has its own objects, stamp and staleness check (_build_lib) and the same flags.  All but
# the last are context-free: one unit without MFMA, the host plumbing of csrc/capi_prelude.hpp, bound by busca_amd/_<stem>_lib.py.  They compile
# kernel includes whole, so an edit to one rebuilds every library named with it here.
LIBS = [
    # device-resident tracker state; shares track_kernel and pairwise_kernel with hip
    ("track", [("busca_track", False)], ["busca_track.h", "busca_hip.h"]),
    # device-resident appearance state; store_kernel alone, shared with no library above
    ("store", [("busca_store", False)], ["busca_store.h"]),
    # association rounds batched across sequences; track's kernel includes (with kalman_store_kernel) under rounds_kernel
    ("rounds", [("busca_rounds", False)], ["busca_rounds.h", "busca_hip.h"]),
    # StrongSORT's device-resident track state; track's kernel includes under sort_kernel
    ("sort", [("busca_sort", False)], ["busca_sort.h", "busca_hip.h"]),
    # a ByteTrack frame on resident state; track's kernel includes under frame_kernel
    ("frame", [("busca_frame", False)], ["busca_frame.h", "busca_hip.h"]),
    # a StrongSORT frame on resident state; sort's and store's kernel includes under sframe_kernel
    ("sframe", [("busca_sframe", False)], ["busca_sframe.h", "busca_hip.h"]),
    # ByteTrack frames of many sequences; frame's kernel includes under mframe_kernel
    ("mframe", [("busca_mframe", False)], ["busca_mframe.h", "busca_frame.h", "busca_hip.h"]),
    # StrongSORT frames of many sequences; sframe's kernel includes and hip's appear_kernel under msframe_kernel
    ("msframe", [("busca_msframe", False)], ["busca_msframe.h", "busca_sframe.h", "busca_appearance.h", "busca_hip.h"]),
    # a GHOST frame on resident state; the kernel includes of hip's GHOST units and store's under gframe_kernel
    ("gframe", [("busca_gframe", False)], ["busca_gframe.h", "busca_ghost.h", "busca_appearance.h", "busca_hip.h"]),
    # GHOST frames of many sequences; gframe's kernel includes under mgframe_kernel
    ("mgframe", [("busca_mgframe", False)], ["busca_mgframe.h", "busca_gframe.h", "busca_ghost.h", "busca_appearance.h", "busca_hip.h"]),
    # the context-bound library (busca_ctx).  busca_dt_aux: the instantiations that crash the vgpr-form pass (see the file)
    ("hip", [("busca_hip", True), ("busca_dt_f32", True), ("busca_dt_f16", True), ("busca_dt_x3", True), ("busca_dt_aux", False),
             ("busca_dtl_f32", True), ("busca_dtl_f16", True), ("busca_dtl_x3", True), ("busca_reid", True), ("busca_assign", False),
             ("busca_appear", False), ("busca_ghost", False), ("busca_ghost_motion", False)],
     ["busca_hip.h", "busca_assign.h", "busca_assign_stages.h", "busca_appearance.h", "busca_ghost.h", "busca_ghost_motion.h", "busca_reid_bn.h",
      "busca_ecc.h"]),
]


def lib_path(stem):
    return os.path.join(HERE, "libbusca_%s.so" % stem)


# TRACK_OUT ... MGFRAME_OUT: the paths the bindings load; OUT, UNITS, HEADERS, STAMP: those of libbusca_hip.so
for _stem, _units, _headers in LIBS[:-1]:
    globals()[_stem.upper() + "_OUT"] = lib_path(_stem)
OUT, (_, UNITS, HEADERS) = lib_path("hip"), LIBS[-1]
STAMP = OUT + ".flags"


def _requested_flags():
    """The flag set this environment asks for (BUSCA_CONV_PROBE, BUSCA_NO_VGPR_FORM change it)."""
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-fvisibility=hidden", "-Wno-unused-value"]
    if os.environ.get("BUSCA_CONV_PROBE"):      # s_memtime phase stamps in the ReID conv kernels (BUSCA_CONV_TS); costs ~1 %, off by default
        flags.append("-DBUSCA_CONV_PROBE")
    if os.environ.get("BUSCA_SPLIT_RELAXED"):   # A/B only: the token-split hand-off without its agent-scope fences (dt_kernel.hip.inc)
        flags.append("-DBUSCA_SPLIT_RELAXED")
    return flags


def _stamp_request():
    return " ".join(_requested_flags()) + (" [no-vgpr-form]" if os.environ.get("BUSCA_NO_VGPR_FORM") is not None else " [vgpr-form if it compiles]")


_INC = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def _deps(path, seen=None):
    """The unit's source and every quoted include below it (recursively)."""
    seen = set() if seen is None else seen
    path = os.path.normpath(path)
    if path in seen or not os.path.exists(path):
        return seen
    seen.add(path)
    for inc in _INC.findall(open(path, errors="replace").read()):
        _deps(os.path.join(os.path.dirname(path), inc), seen)
    return seen


def _newest(paths):
    return max(os.path.getmtime(p) for p in paths)


def _compile(hipcc, unit, vgpr, used_line, verbose):
    """One unit -> build/<unit>.o.  -amdgpu-mfma-vgpr-form: MFMA results land in VGPRs instead of AGPRs, which removes ~1 500 v_accvgpr_* copies from the
    Decision-Transformer kernels (their epilogues are VALU work on the accumulators): f16 DT-step +7 %, f32 +1-2 %, ReID unchanged (measured A/B on
    MI355X, round 2).  The pass behind it is young (it crashed on an experimental variant of the kernel), so a unit that fails to compile with it is
    retried with the plain flags."""
    src, obj = os.path.join(CSRC, unit + ".hip"), os.path.join(OBJ, unit + ".o")
    base = [hipcc] + [f for f in _requested_flags() if f != "-shared"] + ["-c", "-o", obj + ".tmp", src, '-DBUSCA_BUILD_FLAGS="%s"' % used_line]
    tries = [VGPR_FORM, []] if vgpr else [[]]
    r = None
    for extra in tries:
        cmd = base + extra
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode == 0:
            os.replace(obj + ".tmp", obj)
            return unit, bool(extra), r.stderr
        if extra:
            sys.stderr.write("hipcc failed on %s with %s; retrying without it\n" % (unit, " ".join(extra)))
    raise RuntimeError("hipcc failed building %s.o:\n%s%s" % (unit, r.stdout, r.stderr))


def _build_lib(out, units, headers, force, verbose):
    """(Re)build one library: a unit whose object is older than any file it includes, or everything when the library was built for another flag request
    (sidecar stamp <library>.flags: line 1 = the request, line 2 = the flags that compiled - busca_build_info() returns line 2).  Without hipcc
    (a GPU box that received the built library) an existing library is used as it is."""
    stamp = out + ".flags"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    have_hipcc = os.path.exists(hipcc)
    stamp_ok = os.path.exists(stamp) and open(stamp).read().split("\n")[0] == _stamp_request()
    all_deps = set()
    for unit, _ in units:
        all_deps |= _deps(os.path.join(CSRC, unit + ".hip"))
    for h in headers:
        all_deps.add(os.path.join(os.path.dirname(HERE), "include", h))
    if not force and os.path.exists(out) and os.path.getmtime(out) >= _newest(all_deps) and (stamp_ok or not have_hipcc):
        return out
    if not have_hipcc:
        raise RuntimeError("%s is stale or missing and hipcc (%s) is not here" % (out, hipcc))
    os.makedirs(OBJ, exist_ok=True)
    want_vgpr = os.environ.get("BUSCA_NO_VGPR_FORM") is None
    used_line = " ".join(_requested_flags() + (VGPR_FORM if want_vgpr else []))
    stale = []
    for unit, vgpr in units:
        obj = os.path.join(OBJ, unit + ".o")
        if force or not stamp_ok or not os.path.exists(obj) or os.path.getmtime(obj) < _newest(_deps(os.path.join(CSRC, unit + ".hip"))):
            stale.append((unit, vgpr and want_vgpr))
    jobs = int(os.environ.get("BUSCA_BUILD_JOBS", "0")) or min(len(stale) or 1, os.cpu_count() or 4)
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        for unit, with_vgpr, warn in ex.map(lambda uv: _compile(hipcc, uv[0], uv[1], used_line, verbose), stale):
            if verbose and warn.strip():
                sys.stderr.write(warn)
    # the objects carry their device code already (no relocatable device code): a plain host link against the HIP runtime
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")
    clang = clang if os.path.exists(clang) else "/opt/rocm/lib/llvm/bin/clang++"
    cmd = [clang, "-shared", "-fPIC", "--hip-link", "--offload-arch=gfx950", "-o", out + ".tmp"] + [os.path.join(OBJ, u + ".o") for u, _ in units]
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("hipcc failed linking %s" % os.path.basename(out))
    os.replace(out + ".tmp", out)
    with open(stamp, "w") as f:
        f.write(_stamp_request() + "\n" + used_line + "\n")
    return out


def build(force=False, verbose=False):
    """(Re)build what is stale of the libraries of LIBS, each by its own unit list, objects and stamp (_build_lib) -> the path of libbusca_hip.so."""
    for stem, units, headers in LIBS:
        _build_lib(lib_path(stem), units, headers, force, verbose)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
