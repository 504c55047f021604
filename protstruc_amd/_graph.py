"""ctypes binding of libprotstruc_graph.so (C ABI: include/protstruc_graph.h) -- the radius graph, K47 and K48.

A library of its own beside libprotstruc_hip.so, bound the same way: the table is read from the header, and a library
that is missing, older than its sources or of another version is refused -- there is no other code path.
"""
import ctypes
import os

from ._headers import HipLibraryError, prototypes

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libprotstruc_graph.so")
EXPECTED_API = 1  # PS_GRAPH_API of include/protstruc_graph.h; bumped together with any signature change

SIGNATURES = prototypes("protstruc_graph.h")   # name -> (restype, argtypes); a pointer of any kind is a c_void_p

_lib = None


def load():
    """Load the shared library once, type every entry point and check the version."""
    global _lib
    if _lib is not None:
        return _lib
    from . import build

    in_tree = os.path.abspath(LIB_PATH) == os.path.abspath(build.GRAPH_LIB_PATH)
    if in_tree and build.graph_is_stale() and os.path.exists(build.HIPCC) and not os.environ.get("PROTSTRUC_AMD_NO_AUTOBUILD"):
        try:   # missing, or older than its sources: rebuild in place; never a fallback -- if this fails, the checks below raise
            build.build_graph(force=True, verbose=True)
        except Exception as exc:  # noqa: BLE001 -- reported below as "missing" / "older than its sources"
            print(f"[protstruc_amd] in-tree build of libprotstruc_graph.so failed: {exc}", flush=True)
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} is missing: build it with `python -m protstruc_amd.build` "
            "(hipcc --offload-arch=gfx950). protstruc_amd has no CPU fallback.")
    if in_tree and build.graph_is_stale():
        raise HipLibraryError(
            f"{LIB_PATH} is older than its sources (csrc_graph/*.hip, csrc/*.hpp, include/protstruc_graph.h) and could not "
            "be rebuilt here: run `python -m protstruc_amd.build --force` where hipcc is available.")
    lib = ctypes.CDLL(LIB_PATH)
    try:
        lib.ps_graph_api.restype = ctypes.c_int
        api = lib.ps_graph_api()
    except AttributeError as exc:
        raise HipLibraryError(f"{LIB_PATH} does not export ps_graph_api: not a protstruc_amd library") from exc
    if api != EXPECTED_API:
        raise HipLibraryError(f"{LIB_PATH} has radius-graph API version {api}, this package binds version {EXPECTED_API}: "
                              "rebuild with `python -m protstruc_amd.build --force`")
    for name, (restype, argtypes) in SIGNATURES.items():
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
