"""Build libbusca_hip.so, libbusca_track.so, libbusca_store.so, libbusca_rounds.so, libbusca_sort.so, libbusca_frame.so, libbusca_sframe.so, libbusca_mframe.so, libbusca_msframe.so, libbusca_gframe.so and libbusca_mgframe.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

The library is several translation units (csrc/busca_internal.hpp lists them) compiled IN PARALLEL into busca_amd/build/*.o and linked: a full build is
as long as its slowest unit, and an edit recompiles only the units that include the edited file."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
OUT = os.path.join(HERE, "libbusca_hip.so")
STAMP = OUT + ".flags"
# (unit, compiled with -amdgpu-mfma-vgpr-form where that compiles).  busca_dt_aux: the instantiations that crash that pass (see the file).
UNITS = [("busca_hip", True), ("busca_dt_f32", True), ("busca_dt_f16", True), ("busca_dt_x3", True), ("busca_dt_aux", False),
         ("busca_dtl_f32", True), ("busca_dtl_f16", True), ("busca_dtl_x3", True), ("busca_reid", True), ("busca_assign", False), ("busca_appear", False), ("busca_ghost", False), ("busca_ghost_motion", False)]
VGPR_FORM = ["-mllvm", "-amdgpu-mfma-vgpr-form"]
HEADERS = ["busca_hip.h", "busca_assign.h", "busca_assign_stages.h", "busca_appearance.h", "busca_ghost.h", "busca_ghost_motion.h", "busca_reid_bn.h", "busca_ecc.h"]
# libbusca_track.so (include/busca_track.h): the context-free library of device-resident tracker state.  Its own units, objects, stamp and staleness
# check; the same flags, no MFMA in it.  It shares kernel includes with busca_hip (track_kernel, pairwise_kernel), so an edit there rebuilds both.
TRACK_OUT = os.path.join(HERE, "libbusca_track.so")
TRACK_UNITS = [("busca_track", False)]
TRACK_HEADERS = ["busca_track.h", "busca_hip.h"]
# libbusca_store.so (include/busca_store.h): the context-free library of device-resident appearance state.  Handled exactly as the track library; it
# shares no kernel text with the other two.
STORE_OUT = os.path.join(HERE, "libbusca_store.so")
STORE_UNITS = [("busca_store", False)]
STORE_HEADERS = ["busca_store.h"]
# libbusca_rounds.so (include/busca_rounds.h): the context-free library of association rounds batched across sequences.  Handled as the two above; it
# compiles the kernel includes of the track library (and kalman_store_kernel with them), so an edit there rebuilds both.
ROUNDS_OUT = os.path.join(HERE, "libbusca_rounds.so")
ROUNDS_UNITS = [("busca_rounds", False)]
ROUNDS_HEADERS = ["busca_rounds.h", "busca_hip.h"]
# libbusca_sort.so (include/busca_sort.h): the context-free library of StrongSORT's device-resident track state.  Handled as the three above; it
# compiles the kernel includes of the track library under its own sort_kernel, so an edit there rebuilds it too.
SORT_OUT = os.path.join(HERE, "libbusca_sort.so")
SORT_UNITS = [("busca_sort", False)]
SORT_HEADERS = ["busca_sort.h", "busca_hip.h"]
# libbusca_frame.so (include/busca_frame.h): the context-free library of a ByteTrack frame on resident state - the cost slab of the three rounds and
# the match vectors applied to the Kalman state.  Handled as the four above; it compiles the kernel includes of the track library under its own
# frame_kernel, so an edit there rebuilds it too.
FRAME_OUT = os.path.join(HERE, "libbusca_frame.so")
FRAME_UNITS = [("busca_frame", False)]
FRAME_HEADERS = ["busca_frame.h", "busca_hip.h"]
# libbusca_sframe.so (include/busca_sframe.h): the context-free library of a StrongSORT frame on resident state - the camera update with predict, the
# cost slab of Tracker._match and the match vectors applied to the Kalman state and the feature rows.  Handled as the five above; it compiles the kernel
# includes of the sort and store libraries under its own sframe_kernel, so an edit there rebuilds it too.
SFRAME_OUT = os.path.join(HERE, "libbusca_sframe.so")
SFRAME_UNITS = [("busca_sframe", False)]
SFRAME_HEADERS = ["busca_sframe.h", "busca_hip.h"]
# libbusca_mframe.so (include/busca_mframe.h): the context-free library of the ByteTrack frames of many sequences on one store - the ragged batched
# forms of the two calls of libbusca_frame.so.  Handled as the six above; it compiles frame_kernel and the kernel includes below it under its own
# mframe_kernel, so an edit there rebuilds it too.
MFRAME_OUT = os.path.join(HERE, "libbusca_mframe.so")
MFRAME_UNITS = [("busca_mframe", False)]
MFRAME_HEADERS = ["busca_mframe.h", "busca_frame.h", "busca_hip.h"]
# libbusca_msframe.so (include/busca_msframe.h): the context-free library of the StrongSORT frames of many sequences on one store - the ragged batched
# forms of the three calls of libbusca_sframe.so, with the appearance tile of busca_appearance_cost inside the cost kernel.  Handled as the seven
# above; it compiles sframe_kernel, appear_kernel and the kernel includes below them under its own msframe_kernel, so an edit there rebuilds it too.
MSFRAME_OUT = os.path.join(HERE, "libbusca_msframe.so")
MSFRAME_UNITS = [("busca_msframe", False)]
MSFRAME_HEADERS = ["busca_msframe.h", "busca_sframe.h", "busca_appearance.h", "busca_hip.h"]
# libbusca_gframe.so (include/busca_gframe.h): the context-free library of a GHOST frame on resident state - the warp with the motion step, the final
# cost matrix, the threshold filter on the solver's matches and the kept matches applied to the position and feature rings.  Handled as the eight
# above; it compiles the kernel includes of the GHOST units of libbusca_hip.so and of the store library under its own gframe_kernel, so an edit
# there rebuilds it too.
GFRAME_OUT = os.path.join(HERE, "libbusca_gframe.so")
GFRAME_UNITS = [("busca_gframe", False)]
GFRAME_HEADERS = ["busca_gframe.h", "busca_ghost.h", "busca_appearance.h", "busca_hip.h"]
# libbusca_mgframe.so (include/busca_mgframe.h): the context-free library of the GHOST frames of many sequences on one store - the ragged batched
# forms of the four calls of libbusca_gframe.so and of busca_ghost_distance / busca_ghost_thresholds.  Handled as the nine above; it compiles
# gframe_kernel, ghost_kernel and the kernel includes below them under its own mgframe_kernel, so an edit there rebuilds it too.
MGFRAME_OUT = os.path.join(HERE, "libbusca_mgframe.so")
MGFRAME_UNITS = [("busca_mgframe", False)]
MGFRAME_HEADERS = ["busca_mgframe.h", "busca_gframe.h", "busca_ghost.h", "busca_appearance.h", "busca_hip.h"]


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
    """(Re)build what is stale of the eleven libraries, each by its own unit list, objects and stamp (_build_lib) -> the path of libbusca_hip.so."""
    _build_lib(TRACK_OUT, TRACK_UNITS, TRACK_HEADERS, force, verbose)
    _build_lib(STORE_OUT, STORE_UNITS, STORE_HEADERS, force, verbose)
    _build_lib(ROUNDS_OUT, ROUNDS_UNITS, ROUNDS_HEADERS, force, verbose)
    _build_lib(SORT_OUT, SORT_UNITS, SORT_HEADERS, force, verbose)
    _build_lib(FRAME_OUT, FRAME_UNITS, FRAME_HEADERS, force, verbose)
    _build_lib(SFRAME_OUT, SFRAME_UNITS, SFRAME_HEADERS, force, verbose)
    _build_lib(MFRAME_OUT, MFRAME_UNITS, MFRAME_HEADERS, force, verbose)
    _build_lib(MSFRAME_OUT, MSFRAME_UNITS, MSFRAME_HEADERS, force, verbose)
    _build_lib(GFRAME_OUT, GFRAME_UNITS, GFRAME_HEADERS, force, verbose)
    _build_lib(MGFRAME_OUT, MGFRAME_UNITS, MGFRAME_HEADERS, force, verbose)
    return _build_lib(OUT, UNITS, HEADERS, force, verbose)


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
