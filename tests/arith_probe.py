"""ctypes binding of the test-only probe library (tests/native/arith_probe.hip, build/libps_arith_probe.so): one
arithmetic primitive of csrc/ps_common.hpp / csrc/k3_arith.hpp evaluated elementwise over torch CUDA tensors on the
current stream.  For two-argument arms ``a`` is the first argument (y of atan2(y, x), the numerator of a / b)."""
import ctypes
import os

ENTRY = "ps_arith_probe_f32"

# arm name -> (code, number of arguments); the codes are those of the probe source
ARMS = {
    "sqrt_rn_mk": (0, 1), "atan2_ps": (1, 2), "atan2_k3": (2, 2), "acos_ps": (3, 1), "atan2_lib": (4, 2),
    "acos_lib": (5, 1), "div": (6, 2),
    "sqrt_rn_mk_v": (10, 1), "atan2_ps_v": (11, 2), "atan2_k3_v": (12, 2), "acos_ps_v": (13, 1),
    "atan2_k3_vn2": (20, 2), "acos_ps_vn2": (21, 1), "atan2_lib_vn2": (22, 2), "acos_lib_vn2": (23, 1),
    "div_ieee_vn2": (24, 2),
    "atan2_k3_vn4": (30, 2), "acos_ps_vn4": (31, 1), "atan2_lib_vn4": (32, 2), "acos_lib_vn4": (33, 1),
    "div_ieee_vn4": (34, 2),
    "atan2f": (40, 2), "acosf": (41, 1), "sqrtf": (42, 1),
}

# elements one lane owns (2 * NC; 1 for the scalar and library arms)
LANE_ELEMS = {name: (1 if code < 10 or code >= 40 else 2 if code < 20 else 4 if code < 30 else 8)
              for name, (code, _) in ARMS.items()}

# scalar routine -> its packed / multi-column forms, which must equal it bit for bit
FORMS = {
    "sqrt_rn_mk": ("sqrt_rn_mk_v",),
    "atan2_ps": ("atan2_ps_v",),
    "atan2_k3": ("atan2_k3_v", "atan2_k3_vn2", "atan2_k3_vn4"),
    "acos_ps": ("acos_ps_v", "acos_ps_vn2", "acos_ps_vn4"),
    "atan2_lib": ("atan2_lib_vn2", "atan2_lib_vn4"),
    "acos_lib": ("acos_lib_vn2", "acos_lib_vn4"),
    "div": ("div_ieee_vn2", "div_ieee_vn4"),
}

_lib = None


def load():
    """The probe library, built first if it is missing or stale (a no-op when fresh)."""
    global _lib
    if _lib is None:
        from protstruc_amd import build
        lib = ctypes.CDLL(build.build_arith_probe(force=False, verbose=False))
        fn = getattr(lib, ENTRY)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
        _lib = lib
    return _lib


def rocm_version():
    """The installed ROCm's version string (the library the probe's atan2f / acosf / sqrtf come from)."""
    from protstruc_amd import build
    path = os.path.join(os.path.dirname(build.ROCM_LIB.rstrip("/")), ".info", "version")
    try:
        with open(path) as f:
            return f.read().strip()
    except OSError:
        import torch
        return f"unknown (torch.version.hip {torch.version.hip})"


def run(arm, a, b=None, out=None):
    """out[i] = arm(a[i]) or arm(a[i], b[i]) on the current stream: float32 CUDA tensors, contiguous, of one length.
    ``out`` may be a view into a larger buffer (the sentinel tests); a new tensor otherwise."""
    import torch
    code, nargs = ARMS[arm]
    assert a.is_cuda and a.dtype == torch.float32 and a.is_contiguous()
    n = a.numel()
    if nargs == 2:
        assert b is not None and b.is_cuda and b.dtype == torch.float32 and b.is_contiguous() and b.numel() == n
    else:
        assert b is None
    if out is None:
        out = torch.empty_like(a)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n
    rc = load().ps_arith_probe_f32(code, a.data_ptr(), None if b is None else b.data_ptr(), out.data_ptr(), n,
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, f"ps_arith_probe_f32({arm}) returned {rc}"
    return out
