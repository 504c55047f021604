"""ctypes binding of libprotstruc_aggregate.so (C ABI: include/protstruc_aggregate.h) -- message passing on graphs,
K55 - K59: segment reductions, gathers and the edge softmax.

A library of its own beside libprotstruc_hip.so, bound the same way: the table is read from the header, and a library
that is missing, older than its sources or of another version is refused -- there is no other code path.  The names follow
the rule of ``_lib.FAMILIES`` (``ps_aggregate_api``, protstruc_aggregate.h, ``EXPECTED_AGGREGATE_API``), so folding the kernels
into the main library is one line of that registry.
"""
import ctypes
import os

from ._headers import HipLibraryError, prototypes

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libprotstruc_aggregate.so")
EXPECTED_AGGREGATE_API = 1  # PS_AGGREGATE_API of include/protstruc_aggregate.h; bumped together with any signature change

AGGREGATE_SIGNATURES = prototypes("protstruc_aggregate.h")   # name -> (restype, argtypes); a pointer of any kind is a c_void_p

_lib = None


def load():
    """Load the shared library once, type every entry point and check the version."""
    global _lib
    if _lib is not None:
        return _lib
    from . import build

    in_tree = os.path.abspath(LIB_PATH) == os.path.abspath(build.AGGREGATE_LIB_PATH)
    if in_tree and build.aggregate_is_stale() and os.path.exists(build.HIPCC) and not os.environ.get("PROTSTRUC_AMD_NO_AUTOBUILD"):
        try:   # missing, or older than its sources: rebuild in place; never a fallback -- if this fails, the checks below raise
            build.build_aggregate(force=True, verbose=True)
        except Exception as exc:  # noqa: BLE001 -- reported below as "missing" / "older than its sources"
            print(f"[protstruc_amd] in-tree build of libprotstruc_aggregate.so failed: {exc}", flush=True)
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} is missing: build it with `python -m protstruc_amd.build` "
            "(hipcc --offload-arch=gfx950). protstruc_amd has no CPU fallback.")
    if in_tree and build.aggregate_is_stale():
        raise HipLibraryError(
            f"{LIB_PATH} is older than its sources (csrc_aggregate/*.hip, csrc/*.hpp, include/protstruc_aggregate.h) and could "
            "not be rebuilt here: run `python -m protstruc_amd.build --force` where hipcc is available.")
    lib = ctypes.CDLL(LIB_PATH)
    try:
        lib.ps_aggregate_api.restype = ctypes.c_int
        api = lib.ps_aggregate_api()
    except AttributeError as exc:
        raise HipLibraryError(f"{LIB_PATH} does not export ps_aggregate_api: not a protstruc_amd library") from exc
    if api != EXPECTED_AGGREGATE_API:
        raise HipLibraryError(f"{LIB_PATH} has aggregate API version {api}, this package binds version "
                              f"{EXPECTED_AGGREGATE_API}: rebuild with `python -m protstruc_amd.build --force`")
    for name, (restype, argtypes) in AGGREGATE_SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(code, what):
    """HipLibraryError unless ``code`` is hipSuccess; the HIP error's name comes from libprotstruc_hip.so (ps_error_string)"""
    if code != 0:
        from . import _lib as hip
        hip.check(code, what)
