"""Tensor-level wrappers over the C ABI (include/protstruc_hip.h).

Each function takes device tensors, allocates the outputs with PyTorch (the
caller owns every buffer; the library never allocates) and launches on
PyTorch's current HIP stream, so calls order with surrounding torch ops and can
be captured by ``torch.cuda.graph``.  Inputs on the CPU raise: there is no
CPU path in this package.
"""
from __future__ import annotations

import ctypes
import threading
import time
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _aggregate, _csredge, _edgegrad, _lib


RNG_STATE_WORDS = 528  # PS_RNG_STATE_WORDS of include/protstruc_hip.h


def _require_device(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"protstruc_amd: `{name}` lives on {t.device}; the geometry kernels are HIP-only "
            "(no CPU fallback). Move the batch to the GPU first (StructureBatch(..., device='cuda')).")


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    _require_device(t, name)
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    return t.contiguous()


def _f32c_opt(t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    return None if t is None else _f32c(t, name)


def _u8c(t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    """A mask as a contiguous one-byte-per-entry tensor for the kernels, which test every byte against zero (C ABI:
    "any non-zero input byte counts as true"): bool and uint8 tensors are passed as they are -- only their address is
    used, so not even a reinterpreting view is created -- anything else is reduced to its truth value first."""
    if t is None:
        return None
    _require_device(t, name)
    if t.dtype == torch.bool or t.dtype == torch.uint8:
        return t.contiguous()
    return (t != 0).contiguous()


def _check_rng_state(rng_state: Optional[torch.Tensor], device: torch.device) -> None:
    """The kernels atomically update words 1, 2 and 16 + 16 r (r < 32) of ``rng_state`` on the device: anything but a
    contiguous int64 tensor of RNG_STATE_WORDS words on the coordinates' own GPU would be an out-of-bounds (or
    host-pointer) access, so it is refused before the launch."""
    if rng_state is None:
        return
    if not isinstance(rng_state, torch.Tensor) or rng_state.dtype != torch.int64:
        raise ValueError(f"rng_state must be an int64 tensor of {RNG_STATE_WORDS} words")
    if not rng_state.is_cuda or rng_state.device != device:
        raise ValueError(f"rng_state lives on {rng_state.device}, the coordinates on {device}")
    if rng_state.ndim != 1 or rng_state.numel() < RNG_STATE_WORDS or not rng_state.is_contiguous():
        raise ValueError(f"rng_state must be a contiguous 1-D int64 tensor of {RNG_STATE_WORDS} words "
                         f"(got shape {tuple(rng_state.shape)})")


def _diffusion_operands(xyz: torch.Tensor, beta: torch.Tensor, rng_state: Optional[torch.Tensor],
                        noise: Optional[torch.Tensor]):
    """The per-structure ``beta`` and the noise source of one diffusion step of ``xyz``, checked: (beta, noise) as
    contiguous float32; one of ``rng_state`` and ``noise`` is required."""
    B = xyz.shape[0]
    beta = _f32c(beta, "beta")
    if beta.shape != (B,):
        raise ValueError(f"beta must have shape ({B},), got {tuple(beta.shape)}")
    if noise is not None:
        noise = _f32c(noise, "noise")
        if noise.shape != xyz.shape:
            raise ValueError("noise must have the shape of xyz")
    elif rng_state is None:
        raise ValueError("either rng_state or noise is required")
    _check_rng_state(rng_state, xyz.device)
    _same_device(xyz, beta=beta, noise=noise)
    return beta, noise


def _check_atom_slots(A: int, *slots) -> None:
    for slot in slots:
        if not 0 <= int(slot) < A:
            raise ValueError(f"atom slot {slot} outside [0, {A})")


def _same_device(ref: torch.Tensor, **tensors) -> None:
    for name, t in tensors.items():
        if t is not None and t.device != ref.device:
            raise ValueError(f"`{name}` lives on {t.device}, the coordinates on {ref.device}")


def _check_out(t: Optional[torch.Tensor], shape, name: str, device: Optional[torch.device] = None,
               dtype: torch.dtype = torch.float32) -> None:
    """A caller-supplied output is dereferenced by a kernel: shape, dtype, layout and -- unless ``device`` is None, the
    shape-only checkers -- the device are checked before anything is launched."""
    if t is None:
        return
    if (not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype
            or not t.is_contiguous() or (device is not None and t.device != device)):
        raise ValueError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} tensor of shape {tuple(shape)}"
                         + (f" on {device}" if device is not None else ""))


def _is_integer_tensor(t) -> bool:
    return not (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool)


def _check_float_tensor(t, shape, name: str, like: str) -> None:
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)} to match {like}, got {tuple(t.shape)}")
    if not t.dtype.is_floating_point:
        raise ValueError(f"{name} must be a floating-point tensor, got {t.dtype}")


def _check_optional(t, shape, name: str, like: str = "", like_shape=None, integer: bool = False,
                    floating: bool = False) -> None:
    """An operand that may be None: its shape, a tuple -- the message ends "to match ``like`` ``like_shape``" where those are
    given -- and, with ``integer`` or ``floating``, its dtype."""
    if t is None:
        return
    if tuple(t.shape) != shape:
        match = f" to match {like}" + ("" if like_shape is None else f" {like_shape}") if like else ""
        raise ValueError(f"{name} must have shape {shape}{match}, got {tuple(t.shape)}")
    if integer and not _is_integer_tensor(t):
        raise ValueError(f"{name} must be an integer tensor, got {t.dtype}")
    if floating and not t.dtype.is_floating_point:
        raise ValueError(f"{name} must be a floating-point tensor, got {t.dtype}")


MAX_BATCH = 65535   # structures per call: they are one dimension of the grid


def _check_batch(B: int, what: str = "structures") -> None:
    if B > MAX_BATCH:
        raise ValueError(f"at most {MAX_BATCH} {what} per call, got {B}")


def _check_count(n: int, lo: int, hi: Optional[int], what: str) -> None:
    """``lo <= n <= hi`` -- ``hi`` None: no upper limit --, or ValueError: "lo .. hi ``what``, got n", and "at most hi
    ``what``, got n" where ``lo`` is 0.  A power of two from 2^16 on is written 2^k."""
    if n < lo or (hi is not None and n > hi):
        top = "any number of" if hi is None else f"2^{hi.bit_length() - 1}" if hi >= 2 ** 16 and not hi & (hi - 1) else hi
        raise ValueError((f"{lo} .. {top}" if lo else f"at most {top}") + f" {what}, got {n}")


def _float_dims(t, name: str, axes: str, tail: tuple = (3,)) -> tuple:
    """The shape of the floating-point tensor ``t``, which has the axes that ``axes`` names -- "batch, points, 3" -- the last
    of them ``tail``; ValueError otherwise."""
    shape = tuple(t.shape)
    if len(shape) != axes.count(",") + 1 or shape[len(shape) - len(tail):] != tail:
        raise ValueError(f"{name} must have shape ({axes}), got {shape}")
    if not t.dtype.is_floating_point:
        raise ValueError(f"{name} must be a floating-point tensor, got {t.dtype}")
    return shape


def _xyz_dims(xyz, floating: bool = True) -> Tuple[int, int, int]:
    """(B, N, A) of (batch, residues, atoms, 3) coordinates, which are of a floating-point type unless ``floating`` is
    False; ValueError otherwise."""
    shape = tuple(xyz.shape)
    if len(shape) != 4 or shape[3] != 3:
        raise ValueError(f"xyz must have shape (batch, residues, atoms, 3), got {shape}")
    if floating and not xyz.dtype.is_floating_point:
        raise ValueError(f"xyz must be a floating-point tensor, got {xyz.dtype}")
    return shape[:3]


def _points_dims(points, max_points: int) -> Tuple[int, int]:
    """(B, M) of floating-point (batch, points, 3) points within the limits of a launch -- a grid dimension per
    structure, ``max_points`` (a power of two) points in one; ValueError otherwise."""
    shape = tuple(points.shape)
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"points must have shape (batch, points, 3), got {shape}")
    B, M = shape[:2]
    _check_batch(B)
    if M > max_points:
        raise ValueError(f"at most 2^{max_points.bit_length() - 1} points per structure, got {M}")
    if not points.dtype.is_floating_point:
        raise ValueError(f"points must be a floating-point tensor, got {points.dtype}")
    return B, M


_INF = float("inf")


def _check_scalar(value, name: str, rule: str) -> None:
    """``rule`` is "positive" or "non-negative" (both also finite) or "finite"; NaN passes none of them."""
    v = float(value)
    if not (abs(v) < _INF and (rule == "finite" or v > 0 or (v == 0 and rule == "non-negative"))):
        raise ValueError(f"{name} must be {rule}{'' if rule == 'finite' else ' and finite'}, got {value}")


def _row_range(N: int, row_begin: int, row_end: Optional[int], compact: bool):
    """``_lib.row_range`` with the rows checked against [0, N): (row_end, output rows, origin row)."""
    row_end, out_rows, origin = _lib.row_range(N, row_begin, row_end, compact)
    if not (0 <= row_begin <= row_end <= N):
        raise ValueError(f"row range [{row_begin},{row_end}) outside [0,{N})")
    return row_end, out_rows, origin


def _require_f32c(t: torch.Tensor, name: str, message: str) -> None:
    """An operand a kernel reads or updates where it lies: on the GPU, float32 and contiguous, or ValueError(message)."""
    _require_device(t, name)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(message)


def _launch(name: str, *args) -> None:
    """Call entry point ``name`` of the library; HipLibraryError if it does not return hipSuccess."""
    rc = getattr(_lib.load(), name)(*args)
    if rc:
        _lib.check(rc, name)


def _ptr(t: Optional[torch.Tensor]):
    # a plain int is what ctypes wants for a c_void_p argument (None = NULL); no wrapper object per pointer
    return None if t is None else t.data_ptr()


# torch's current HIP stream of a device as a raw handle: the private accessor torch's own kernel launchers use
# (0.1 us) where it exists, else the public Stream object (1.2 us per call)
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t: torch.Tensor):
    if _raw_stream is not None:
        return _raw_stream(t.device.index)
    return torch.cuda.current_stream(t.device).cuda_stream


class _NoSwitch:
    """`with` target used when the tensor's device is already the current one (the common case): entering
    torch.cuda.device() costs two device switches, about a quarter of a small call's host time."""

    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def _on(device: torch.device):
    """Context that makes ``device`` current for allocations and launches."""
    return _NO_SWITCH if device.index == torch.cuda.current_device() else torch.cuda.device(device)


# ---- optional, per-device choice of K1's output granule per workgroup -----------------------------------------
# How fast K1's store stream is absorbed depends on the physical memory behind the output buffers (DESIGN.md section 4,
# "the two classes of allocation": 6.2-7.3 TB/s for the same kernel on different allocations of one process), and so
# does which launch configuration is the fastest.  The library default (ps_k1_config_default: 32-residue tiles, idle LDS by
# chain length -- 36 KB = 3 workgroups per CU from 256 residues on, 20 KB = 5 below) is the configuration that won on seven
# of eight boxes in round 4 (profiles/r04_k1_tuner_tables.log);
# nothing is timed behind the caller's back.  The tuner is an explicit call -- ops.autotune_pairwise_distance(), which
# bench.py makes before its warm-up and reports -- or, with PROTSTRUC_AMD_AUTOTUNE=1 (read at import;
# ops.set_implicit_autotune at run time), runs on the first large call of each kind per device.  It writes that DEVICE's
# entry of the host-side table in _lib.py (a per-call argument to the library; other devices and threads are never
# affected) and never runs during stream capture.  History of the candidates: NOTES.md.
_K1_TUNED = {}
_K1_TUNE_LOCK = threading.Lock()
import os as _os
_AUTOTUNE_ENV = bool(_os.environ.get("PROTSTRUC_AMD_AUTOTUNE"))   # read once, at import: the launch path does no environment lookups


def set_implicit_autotune(flag: bool) -> None:
    """Opt in to (or out of) tuning K1's launch configuration on the first large call of each kind per device -- what
    ``PROTSTRUC_AMD_AUTOTUNE=1`` in the environment at import time selects.  Off by default."""
    global _AUTOTUNE_ENV
    _AUTOTUNE_ENV = bool(flag)


def _k1_launch_entry(*args):
    """First call: bind the library's entry point, then replace this trampoline with it."""
    global _K1_LAUNCH
    _K1_LAUNCH = _lib.load().ps_pairwise_distance_cfg_f32
    return _K1_LAUNCH(*args)


_K1_LAUNCH = _k1_launch_entry
# K1 kernel dispatches this process has issued through this module (every launch is exactly one kernel dispatch, the
# autotuner's included): bench.py reports the ordinals of its timed launches so that a rocprofv3 kernel trace of the same
# process can be cut at exactly those dispatches (tools/summarize_rocprof.py ranges)
K1_DISPATCHES = [0]
# Candidates of the explicit tuner, as ps_k1_config fields.  The default comes first: the choice moves away from it
# only for a clear (>= 1 %) gain in the MEAN launch time.  Pattern kernel (N % 16 == 0): KB of idle LDS per workgroup
# (only lowers the number of resident workgroups per CU: fewer concurrent store streams) and column residues per tile.
# Around the default -- 32-residue tiles at 5 workgroups per CU -- sit 4 per CU (24 KB: +1 % on slow buffers and on some
# fast ones, -3 % on others), 6 per CU (16 KB), 3 per CU (36 KB: +1-4 % on slow and medium buffers, -4 % on fast ones), the
# 16-residue tile, the 64-residue tile and the 128-residue tile + 8 KB that was the default until late round 3
# (profiles/r03_k1_ab_lean_*.log).
# Round 4: 36 KB won on seven of eight boxes at B=64, N=512 (1.5-3.8 %; profiles/r04_k1_tuner_tables.log) and is what the
# library default (-1: by chain length) now takes from 256 residues on; 20 KB stays a candidate.
_K1_CANDIDATE_PATTERN = (
    {"rows_per_block": 1, "lds_pad_kb": -1, "jt": 0},      # the default: 32-residue tiles, idle LDS by chain length (36 KB = 3 workgroups per CU from N = 256, 20 KB = 5 below)
    {"rows_per_block": 1, "lds_pad_kb": 20, "jt": 32},
    {"rows_per_block": 1, "lds_pad_kb": 24, "jt": 32},
    {"rows_per_block": 1, "lds_pad_kb": 16, "jt": 32},
    {"rows_per_block": 1, "lds_pad_kb": 36, "jt": 32},
    {"rows_per_block": 1, "lds_pad_kb": 0, "jt": 16},
    {"rows_per_block": 1, "lds_pad_kb": 20, "jt": 64},
    {"rows_per_block": 1, "lds_pad_kb": 8, "jt": 128},
)
# flat kernel (any other N >= 16): chunks per workgroup, KB of idle LDS
# (round 3: 32-pair chunks -- 36 KB per short-lived workgroup, 4 workgroups per CU -- run 6.1-6.3 TB/s on every buffer:
# 3-5 % ahead of the 128-pair default on slow buffers, 13 % behind on fast ones; profiles/r03_k1_ab_small_granule.log)
_K1_CANDIDATE_FLAT = (
    {"flat_cpw": 1, "flat_lds_pad_kb": 0, "flat_fl_log2": 0},      # the default: 64-pair chunks
    {"flat_cpw": 1, "flat_lds_pad_kb": 8, "flat_fl_log2": 0},
    {"flat_cpw": 1, "flat_lds_pad_kb": 0, "flat_fl_log2": 7},
    {"flat_cpw": 2, "flat_lds_pad_kb": 0, "flat_fl_log2": 0},
    {"flat_cpw": 1, "flat_lds_pad_kb": 0, "flat_fl_log2": 5},
)


def _cand_label(c) -> str:
    if "rows_per_block" in c:
        pad = "+autoKB" if c["lds_pad_kb"] < 0 else (f"+{c['lds_pad_kb']}KB" if c["lds_pad_kb"] else "")
        return f"{c['rows_per_block']}row" + pad + (f" jt{c['jt']}" if c["jt"] else "")
    return f"{c['flat_cpw']}chunk" + (f"+{c['flat_lds_pad_kb']}KB" if c["flat_lds_pad_kb"] else "") + \
        (f" {1 << c['flat_fl_log2']}pairs" if c.get("flat_fl_log2") else "")


def _autotune_k1(device, args, n_pairs: int, N: int, A: int, force: bool = False) -> None:
    if not force and not _AUTOTUNE_ENV:   # (the hot path does not even get here: see the caller)
        return
    if A != 15 or N < 16 or n_pairs < (1 << 22):
        return
    # which kernel this shape takes decides which knob is tuned (pairwise_distance.hip: flat_eligible)
    pattern = (N % 16 == 0)
    result_key = "rows_per_block" if pattern else "flat_cpw"
    if result_key in _K1_TUNED.get(device, {}):
        return
    if torch.cuda.is_current_stream_capturing():
        return
    if not pattern and (_lib.get_tuning("k1_flat", device) == 0 or _lib.get_tuning("k1_variant", device) != 0):
        return
    with _K1_TUNE_LOCK:
        if result_key in _K1_TUNED.get(device, {}):   # another thread tuned this device while we waited
            return
        lib = _lib.load()
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        candidates = _K1_CANDIDATE_PATTERN if pattern else _K1_CANDIDATE_FLAT
        if pattern:
            # candidate 0 (lds_pad_kb = -1, jt = 0) resolves to {36 KB from N = 256, 20 KB below; 32-residue tiles}
            # (pairwise_distance.hip, launch_a15): the explicit candidate that names the same launch is not timed -- a "pick"
            # between two names of one launch would be noise and would make bench.py re-time the default for nothing
            alias = {"rows_per_block": 1, "lds_pad_kb": 36 if N >= 256 else 20, "jt": 32}
            candidates = tuple(c for c in candidates if c != alias)
        # one private configuration struct per candidate: nothing shared is touched while timing
        cfgs = [_lib.k1_config(device, **c) for c in candidates]

        def launch(k):
            K1_DISPATCHES[0] += 1
            _lib.check(lib.ps_pairwise_distance_cfg_f32(*args, ctypes.byref(cfgs[k]), stream),
                       "ps_pairwise_distance_cfg_f32 (autotune)")

        # the first ~70 ms of GPU work after idle run ~2.5 % slow (clock ramp): warm up before timing anything,
        # then time the candidates in interleaved rounds
        t_end = time.perf_counter() + 0.12
        while time.perf_counter() < t_end:
            launch(0)
            torch.cuda.current_stream(device).synchronize()
        # Each candidate's figure is its MEAN over all rounds (5 x 3 launches), not its minimum or median: the small-tile
        # kernels spread 3-4 % from launch to launch with a tail of slow launches (profiles/r03_k1_launch_series.log;
        # a median of 2.60 ms went with a 20-launch mean of 2.72 ms in profiles/r03_final_bench_n1.json), and a caller's
        # throughput is the reciprocal of the mean.
        rounds = [[] for _ in candidates]
        for _ in range(5):
            for k in range(len(candidates)):
                launch(k)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(k)
                launch(k)
                launch(k)
                e1.record()
                e1.synchronize()
                rounds[k].append(e0.elapsed_time(e1) / 3)
        timings = [sum(r) / len(r) for r in rounds]
        best = 0
        for k in range(1, len(candidates)):
            if timings[k] < timings[best] * 0.99:   # prefer the earlier candidate unless the gain is clear (1 %)
                best = k
        for field, value in candidates[best].items():
            _lib.set_tuning("k1_" + field, value, device)
        report = dict(candidates[best])
        report["flat_ms" if not pattern else "ms"] = {_cand_label(c): timings[k] for k, c in enumerate(candidates)}
        _K1_TUNED.setdefault(device, {}).update(report)


def set_exact_sqrt(flag: bool, device=None) -> None:
    """K1 arithmetic on ``device`` (default: the current one).  Both modes take the squared length as the reference's
    torch.norm does, fma(dz, dz, fma(dy, dy, dx * dx)).  False (default) = hardware square root, exact for 85 % of inputs
    and 1 ulp off for the rest, so within 1 ulp of the reference; True = correctly rounded square root, the reference's
    bits (slower on fast allocations).
    ``PROTSTRUC_AMD_EXACT_SQRT=1`` in the environment makes True the default of every device."""
    _lib.set_tuning("k1_exact_sqrt", 1 if flag else 0, device)


def get_exact_sqrt(device=None) -> bool:
    return bool(_lib.get_tuning("k1_exact_sqrt", device))


def set_exact_angles(flag: bool, device=None) -> None:
    """K3 / featuriser arithmetic on ``device`` (default: the current one).  False (default): the fast forms -- exact
    where the reference is exact, otherwise within the conditioning gates (3.8e-6 of off-diagonal dihedrals more than
    1e-5 from the reference at unit scale).  True: geometry.dihedral / geometry.angle in the reference's order of
    operations (three np.cross-form cross products, torch.norm's fused squared length, IEEE division by |b1|, library
    atan2 / acos): everything up to the atan2 / acos argument is the reference's bits, and no entry is beyond 1e-5, on
    the same per-CU sweep kernels as the fast forms (DESIGN.md section 4 has both modes' times).  ``PROTSTRUC_AMD_EXACT_ANGLES=1`` makes True the default of every device."""
    _lib.set_exact_angles(flag, device)


def get_exact_angles(device=None) -> bool:
    return bool(_lib.get_exact_angles(device))


def exact_sqrt(flag: bool = True, device=None):
    """``with ops.exact_sqrt():`` -- ``set_exact_sqrt(flag, device)`` for the length of the block; on exit the device's
    settings are what they were on entry (``_lib.scoped_settings``: for tests and tools, not for concurrent threads)."""
    return _lib.scoped_settings(device, k1_exact_sqrt=1 if flag else 0)


def exact_angles(flag: bool = True, device=None):
    """``with ops.exact_angles():`` -- ``set_exact_angles(flag, device)`` for the length of the block (see ``exact_sqrt``)."""
    return _lib.scoped_settings(device, exact_angles=flag)


def k1_tuning(device=None, **knobs):
    """``with ops.k1_tuning(jt=16, lds_pad_kb=0):`` -- K1 launch knobs, named like the ``_lib.k1_config`` overrides
    (no ``k1_`` prefix), for the length of the block (see ``exact_sqrt``).  A ``_lib.set_tuning`` inside the block is
    undone on exit too, so a sweep can step a knob in a loop under one enclosing scope."""
    return _lib.scoped_settings(device, **{"k1_" + name: value for name, value in knobs.items()})


def autotune_pairwise_distance(xyz: torch.Tensor, atom_mask: Optional[torch.Tensor], out_dist: torch.Tensor,
                               out_mask: torch.Tensor):
    """Time K1's launch configurations on the given buffers now and keep the fastest for this device (results are
    identical for every configuration).  Optional: the default configuration is already the one that was fastest on
    every buffer measured."""
    pairwise_distance(xyz, atom_mask, out_dist=out_dist, out_mask=out_mask, _autotune=True)
    torch.cuda.current_stream(xyz.device).synchronize()
    return k1_autotune_result(xyz.device)


def allocate_fast_outputs(xyz: torch.Tensor, atom_mask: Optional[torch.Tensor] = None, candidates: int = 4):
    """Output buffers for ``pairwise_distance(..., out_dist=, out_mask=)``, chosen as the fastest of ``candidates``
    fresh allocations.

    Why this exists: on MI355X the rate at which K1's store stream is absorbed depends on which physical memory the
    output landed in -- 6.0 to 7.1 TB/s for the same kernel in one process ("fast and slow
    allocations") -- and a caller who keeps its output buffers for many steps inherits that luck for the whole run.
    This helper allocates the (dist, mask) pair ``candidates`` times (all held at once: candidates x 1125 B per
    residue pair; fewer if the device runs out of memory), times nine launches on each (three interleaved rounds), returns the fastest pair and releases the others.
    Returns ``(dist, mask, report)``; results written into the buffers are the same whichever pair is chosen."""
    xyz = _f32c(xyz, "xyz")
    B, N, A = xyz.shape[:3]
    shape = (B, N, N, A, A)
    pairs = []
    with _on(xyz.device):
        for _ in range(max(1, int(candidates))):
            try:
                d_ = torch.empty(shape, dtype=torch.float32, device=xyz.device)
                pairs.append((d_, torch.empty(shape, dtype=torch.bool, device=xyz.device)))
            except torch.cuda.OutOfMemoryError:      # a shape that does not fit `candidates` times: choose among what did fit
                d_ = None
                if not pairs:
                    raise
                break
        pairwise_distance(xyz, atom_mask, out_dist=pairs[0][0], out_mask=pairs[0][1])   # warm-up
        t_end = time.perf_counter() + 0.12
        while time.perf_counter() < t_end:
            pairwise_distance(xyz, atom_mask, out_dist=pairs[0][0], out_mask=pairs[0][1])
            torch.cuda.current_stream(xyz.device).synchronize()
        ms = [0.0] * len(pairs)   # mean over 3 interleaved rounds of 3 launches (the tuner's statistic, for the same reason)
        for _ in range(3):
            for k, (d, m) in enumerate(pairs):
                pairwise_distance(xyz, atom_mask, out_dist=d, out_mask=m)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _r in range(3):
                    pairwise_distance(xyz, atom_mask, out_dist=d, out_mask=m)
                e1.record()
                e1.synchronize()
                ms[k] += e0.elapsed_time(e1) / 9
        best = min(range(len(pairs)), key=lambda k: ms[k])
        d, m = pairs[best]
        del pairs
        torch.cuda.empty_cache()
    return d, m, {"ms_per_candidate": ms, "chosen": best}


def k1_autotune_result(device=None):
    """What the one-time K1 autotune chose on ``device`` (None if it has not run)."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return _K1_TUNED.get(device)


def pairwise_distance(xyz: torch.Tensor, atom_mask: Optional[torch.Tensor] = None, *,
                      row_begin: int = 0, row_end: Optional[int] = None, compact: bool = False,
                      out_dist: Optional[torch.Tensor] = None, out_mask: Optional[torch.Tensor] = None,
                      want_dist: bool = True, want_mask: bool = True,
                      _autotune: bool = False) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """K1.  Returns (dist fp32, dist_mask bool) of shape (B, rows, N, A, A).

    rows = N for the default full matrix.  With ``row_begin/row_end`` only those
    residue rows are computed: into a compact (B, row_end-row_begin, N, A, A)
    buffer if ``compact`` else into rows [row_begin,row_end) of a full-size
    buffer (``out_dist`` / ``out_mask`` may supply that buffer, e.g. the
    destination of an all-gather)."""
    xyz = _f32c(xyz, "xyz")
    B, N, A = xyz.shape[:3]
    row_end, out_rows, origin = _row_range(N, row_begin, row_end, compact)
    shape = (B, out_rows, N, A, A)
    mask_u8 = _u8c(atom_mask, "atom_mask")
    _same_device(xyz, atom_mask=mask_u8)
    # caller-supplied outputs are dereferenced by a kernel launched on xyz.device: a CPU tensor or a tensor of another
    # GPU would be a wild device write, so device, shape, dtype and layout are all checked before anything is launched
    if want_dist:
        _check_out(out_dist, shape, "out_dist", xyz.device)
    if want_mask:
        _check_out(out_mask, shape, "out_mask", xyz.device, torch.bool)
    with _on(xyz.device):
        dist = dmask = None
        if want_dist:
            dist = out_dist if out_dist is not None else torch.empty(shape, dtype=torch.float32, device=xyz.device)
        if want_mask:
            dmask = out_mask if out_mask is not None else torch.empty(shape, dtype=torch.bool, device=xyz.device)
        args = (_ptr(xyz), _ptr(mask_u8), _ptr(dist), _ptr(dmask), B, N, A, row_begin, row_end, out_rows, origin)
        if _autotune or _AUTOTUNE_ENV:
            _autotune_k1(xyz.device, args, B * (row_end - row_begin) * N, N, A, force=_autotune)
        cfg_ref = _lib.k1_config_ref(xyz.device.index)   # this device's settings, snapshotted for this launch
        rc = 0
        if not (B == 0 or N == 0 or row_begin == row_end):   # empty input: nothing to launch (an empty tensor has no device pointer)
            K1_DISPATCHES[0] += 1
            rc = _K1_LAUNCH(*args, cfg_ref, _stream(xyz))
    if rc:
        _lib.check(rc, "ps_pairwise_distance_cfg_f32")
    return dist, dmask


def backbone_dihedrals(xyz: torch.Tensor, chain_idx: torch.Tensor, residue_mask: torch.Tensor, *,
                       want_dihedrals: bool = True, want_mask: bool = True, want_nterm: bool = True,
                       want_cterm: bool = True):
    """K2.  Returns (dihedrals (B,N,3) fp32, dihedral_mask (B,N,3) bool, nterm (B,N) bool, cterm (B,N) bool);
    an output that is not wanted is neither allocated nor written and comes back as None."""
    xyz = _f32c(xyz, "xyz")
    B, N, A = xyz.shape[:3]
    chain = _f32c(chain_idx, "chain_idx")
    rmask = _u8c(residue_mask, "residue_mask")
    dev = xyz.device
    if not (want_dihedrals or want_mask or want_nterm or want_cterm):
        raise ValueError("at least one output must be requested")
    with _on(dev):
        dih = torch.empty(B, N, 3, dtype=torch.float32, device=dev) if want_dihedrals else None
        dmask = torch.empty(B, N, 3, dtype=torch.bool, device=dev) if want_mask else None
        nterm = torch.empty(B, N, dtype=torch.bool, device=dev) if want_nterm else None
        cterm = torch.empty(B, N, dtype=torch.bool, device=dev) if want_cterm else None
        if not (B == 0 or N == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_backbone_dihedrals_f32", _ptr(xyz), _ptr(chain), _ptr(rmask), _ptr(dih), _ptr(dmask),
                    _ptr(nterm), _ptr(cterm), B, N, A, _stream(xyz))
    return dih, dmask, nterm, cterm


def pairwise_angles(xyz: torch.Tensor, slots_i: Sequence[int], slots_j: Sequence[int], n_points: int, *,
                    row_begin: int = 0, row_end: Optional[int] = None, compact: bool = False,
                    out: Optional[torch.Tensor] = None, _one_column: bool = False) -> torch.Tensor:
    """K3.  n_points = 4: dihedral, 3: planar angle, over points (slots_i of residue i ++ slots_j of residue j).
    Only residue rows [row_begin, row_end) are computed, with K1's row addressing: into rows [row_begin, row_end) of
    a full-size (B, N, N) buffer (``out`` may supply it, e.g. the destination of an all-gather) or, with ``compact``,
    into a (B, row_end - row_begin, N) buffer.  ``_one_column`` (tests): the device's arithmetic (``set_exact_angles``)
    through the simple one-column kernel at any shape (bit 1 of ``exact_angles`` of the C ABI, diagnostic)."""
    xyz = _f32c(xyz, "xyz")
    B, N, A = xyz.shape[:3]
    slots = [int(s) for s in slots_i] + [int(s) for s in slots_j]
    src = [0] * len(slots_i) + [1] * len(slots_j)
    if len(slots) < n_points:
        raise IndexError(f"need {n_points} atoms in total, got {len(slots)}")  # the reference indexes past the end
    slots, src = slots[:n_points], src[:n_points]
    row_end, out_rows, origin = _row_range(N, row_begin, row_end, compact)
    arr = ctypes.c_int * n_points
    with _on(xyz.device):
        if out is None:
            out = torch.empty(B, out_rows, N, dtype=torch.float32, device=xyz.device)
        else:
            _check_out(out, (B, out_rows, N), "out", xyz.device)
        if not (B == 0 or N == 0 or row_begin == row_end):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_pairwise_angles_f32", _ptr(xyz), _ptr(out), B, N, A, n_points, arr(*src), arr(*slots),
                    row_begin, row_end, out_rows, origin, _lib.get_exact_angles(xyz.device) | (2 if _one_column else 0),
                    _stream(xyz))
    return out


def inter_residue_geometry(xyz: torch.Tensor, atom_mask: Optional[torch.Tensor] = None, *, _one_column: bool = False):
    """Fused featuriser: dict of six (B,N,N) fp32 planes and three (B,N,N) bool planes.  The distance planes use the
    device's K1 square-root mode (``set_exact_sqrt``), so they equal the slices of ``pairwise_distance`` bit for bit."""
    xyz = _f32c(xyz, "xyz")
    B, N, A = xyz.shape[:3]
    if A < 5:
        raise IndexError("inter_residue_geometry needs the N, CA, C, O, CB atom slots")

    m = _u8c(atom_mask, "atom_mask")
    dev = xyz.device
    fkeys = ["d_ca", "d_cb", "d_no", "omega", "theta", "phi"]
    mkeys = ["d_ca_mask", "d_cb_mask", "d_no_mask"]
    with _on(dev):
        # nine planes in two allocations, every plane on a 16-byte boundary (plane stride padded): the kernel's flat mask
        # stores then share one 16-byte grid and decode each group once for the three mask planes (any N)
        plane = B * N * N
        fstride, kstride = (plane + 3) & ~3, (plane + 15) & ~15
        f = torch.empty(6, fstride, dtype=torch.float32, device=dev)
        k = torch.empty(3, kstride, dtype=torch.bool, device=dev)
        if not (B == 0 or N == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            fp, kp = f.data_ptr(), k.data_ptr()                       # plane addresses by arithmetic, not by 9 views
            _launch("ps_inter_residue_geometry_f32", _ptr(xyz), _ptr(m), *[fp + 4 * fstride * i for i in range(6)],
                    *[kp + kstride * i for i in range(3)], B, N, A, _lib.get_tuning("k1_exact_sqrt", dev),
                    _lib.get_exact_angles(dev) | (2 if _one_column else 0), _stream(xyz))
    out = {key: f[i, :plane].view(B, N, N) for i, key in enumerate(fkeys)}
    out.update({key: k[i, :plane].view(B, N, N) for i, key in enumerate(mkeys)})
    return out


IRG_GRAD_KEYS = ("d_ca", "d_cb", "d_no", "omega", "theta", "phi")   # the differentiable planes, in the C ABI's order
IRG_BACKWARD_MAX_N = 2048   # the backward kernel stages a structure's used slots in LDS (include/protstruc_hip.h)


def check_inter_residue_geometry_backward_shapes(xyz, grads, atom_mask=None, out=None) -> None:
    """Shape rules of ``inter_residue_geometry_backward``, on shapes and dtypes only (no device, no launch): KeyError for
    a key of ``grads`` that is no float plane, ValueError for a wrong rank or shape, IndexError for fewer than five atom
    slots (as the forward raises)."""
    for key in grads:
        if key not in IRG_GRAD_KEYS:
            raise KeyError(f"{key!r} is not a differentiable plane of inter_residue_geometry (known: {', '.join(IRG_GRAD_KEYS)})")
    B, N, A = _xyz_dims(xyz)
    shape = (B, N, A, 3)
    if A < 5:
        raise IndexError("inter_residue_geometry needs the N, CA, C, O, CB atom slots")
    if N > IRG_BACKWARD_MAX_N:
        raise ValueError(f"inter_residue_geometry_backward takes at most {IRG_BACKWARD_MAX_N} residues, got {N}")
    _check_optional(atom_mask, (B, N, A), "atom_mask", "xyz", shape)
    for key, g in grads.items():
        if g is not None:
            _check_float_tensor(g, (B, N, N), f"grads[{key!r}]", f"xyz {shape}")
    _check_out(out, shape, "out")


def inter_residue_geometry_backward(xyz: torch.Tensor, grads, atom_mask: Optional[torch.Tensor] = None, *,
                                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Vector-Jacobian product of the fused featuriser in one launch: ``grad_xyz`` (B,N,A,3) fp32 with
    ``grad_xyz[b, r, s] = sum over planes and (i, j) of grads[plane][b, i, j] * d plane[b, i, j] / d xyz[b, r, s]``.
    ``grads`` maps any subset of d_ca / d_cb / d_no / omega / theta / phi to (B,N,N) upstream gradients (a missing key or
    a None value means zero; anything not contiguous fp32 is made so).  Entries that read an atom absent from
    ``atom_mask``, and the diagonal of every plane but d_no, contribute exactly zero -- NaN coordinates and NaN upstream
    values there never reach the result (include/protstruc_hip.h).  Every element of ``out`` is written (exact zeros in
    the slots the featuriser does not read); deterministic; independent of ``set_exact_sqrt`` / ``set_exact_angles``."""
    check_inter_residue_geometry_backward_shapes(xyz, grads, atom_mask, out)
    xyz = _f32c(xyz, "xyz")
    _same_device(xyz, atom_mask=atom_mask, out=out, **{f"grads[{k!r}]": g for k, g in grads.items()})
    m = _u8c(atom_mask, "atom_mask")
    gs = [None if grads.get(key) is None else _f32c(grads[key], f"grads[{key!r}]") for key in IRG_GRAD_KEYS]
    B, N, A = xyz.shape[:3]
    with _on(xyz.device):
        if out is None:
            out = torch.empty(B, N, A, 3, dtype=torch.float32, device=xyz.device)
        if not (B == 0 or N == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_inter_residue_geometry_backward_f32", _ptr(xyz), _ptr(m), *[_ptr(g) for g in gs], _ptr(out), B,
                    N, A, _stream(xyz))
    return out


def pointwise(mode: int, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, d: Optional[torch.Tensor] = None):
    """angle (mode 0) / dihedral (1) / gram_schmidt (2) / place_fourth_atom (3, ``d`` packed [length, planar, dihedral])
    over broadcast (*,3) tensors."""
    pts = [a, b, c] + ([d] if d is not None else [])
    pts = torch.broadcast_tensors(*[_f32c(p, "points") for p in pts])
    shape = pts[0].shape[:-1]
    if pts[0].shape[-1] != 3:
        raise ValueError("points must have a trailing axis of size 3")
    flat = [p.reshape(-1, 3).contiguous() for p in pts]
    n = flat[0].shape[0]
    dev = flat[0].device
    with _on(dev):
        out = torch.empty({2: (n, 9), 3: (n, 3)}.get(mode, (n,)), dtype=torch.float32, device=dev)
        if not (n == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_pointwise_f32", mode, _ptr(flat[0]), _ptr(flat[1]), _ptr(flat[2]),
                    _ptr(flat[3]) if mode in (1, 3) else None, _ptr(out), n, _stream(flat[0]))
    if mode == 2:
        return out.reshape(*shape, 3, 3)
    return out.reshape(*shape, 3) if mode == 3 else out.reshape(shape)


def check_backbone_from_dihedrals_shapes(dihedrals, chain_idx=None, residue_mask=None, bond_angles=None,
                                         bond_lengths=None) -> None:
    """Shape rules of ``backbone_from_dihedrals``, on shapes only (no device, no launch): ValueError on a mismatch."""
    shape = tuple(dihedrals.shape)
    if len(shape) != 3 or shape[-1] != 3:
        raise ValueError(f"dihedrals must have shape (batch, residues, 3) [phi, psi, omega], got {shape}")
    for name, t, want in (("chain_idx", chain_idx, shape[:2]), ("residue_mask", residue_mask, shape[:2]),
                          ("bond_angles", bond_angles, shape), ("bond_lengths", bond_lengths, shape)):
        _check_optional(t, want, name, "dihedrals", shape)


def backbone_from_dihedrals(dihedrals: torch.Tensor, chain_idx: Optional[torch.Tensor] = None,
                            residue_mask: Optional[torch.Tensor] = None, bond_angles: Optional[torch.Tensor] = None,
                            bond_lengths: Optional[torch.Tensor] = None, include_cb: bool = False, n_slots: int = 15):
    """K7.  Backbone coordinates from (B,N,3) [phi, psi, omega]: returns xyz (B,N,n_slots,3) with N / CA / C in slots
    0-2 (and CB in slot 4 when ``include_cb``), zeros elsewhere, and atom_mask (B,N,n_slots) float32 1 / 0.  Optional
    per-residue (B,N) chain_idx / residue_mask start new segments; optional (B,N,3) bond_angles / bond_lengths override
    the ideal geometry (include/protstruc_hip.h)."""
    check_backbone_from_dihedrals_shapes(dihedrals, chain_idx, residue_mask, bond_angles, bond_lengths)
    if n_slots < (5 if include_cb else 3):
        raise ValueError(f"n_slots = {n_slots} leaves no room for {'N, CA, C and CB' if include_cb else 'N, CA, C'}")
    dih = _f32c(dihedrals, "dihedrals")
    _same_device(dih, chain_idx=chain_idx, residue_mask=residue_mask, bond_angles=bond_angles, bond_lengths=bond_lengths)
    chain, rmask = _f32c_opt(chain_idx, "chain_idx"), _u8c(residue_mask, "residue_mask")
    ang, lens = _f32c_opt(bond_angles, "bond_angles"), _f32c_opt(bond_lengths, "bond_lengths")
    B, N = dih.shape[:2]
    dev = dih.device
    with _on(dev):
        xyz = torch.empty(B, N, n_slots, 3, dtype=torch.float32, device=dev)
        atom_mask = torch.empty(B, N, n_slots, dtype=torch.float32, device=dev)
        if not (B == 0 or N == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_backbone_from_dihedrals_f32", _ptr(dih), _ptr(ang), _ptr(lens), _ptr(chain), _ptr(rmask),
                    _ptr(xyz), _ptr(atom_mask), int(bool(include_cb)), B, N, n_slots, _stream(dih))
    return xyz, atom_mask


def check_backbone_from_dihedrals_backward_shapes(xyz, grad_xyz, chain_idx=None, residue_mask=None, include_cb=False,
                                                  want_bond_angles=False, want_bond_lengths=False, out=None) -> None:
    """Shape rules of ``backbone_from_dihedrals_backward``, on shapes and dtypes only (no device, no launch): ValueError."""
    B, N, A = _xyz_dims(xyz)
    shape = (B, N, A, 3)
    _check_float_tensor(grad_xyz, shape, "grad_xyz", "xyz")
    if A < (5 if include_cb else 3):
        raise ValueError(f"{A} atom slots leave no room for {'N, CA, C and CB' if include_cb else 'N, CA, C'}")
    _check_optional(chain_idx, (B, N), "chain_idx", "xyz", shape)
    _check_optional(residue_mask, (B, N), "residue_mask", "xyz", shape)
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 3:
            raise ValueError("out must be a (grad_dihedrals, grad_bond_angles, grad_bond_lengths) triple (None where not wanted)")
        for name, t, wanted in (("out[0]", out[0], True), ("out[1]", out[1], want_bond_angles), ("out[2]", out[2], want_bond_lengths)):
            if t is not None and not wanted:
                raise ValueError(f"{name} is given but that gradient is not wanted")
            _check_out(t, (B, N, 3), name)


def backbone_from_dihedrals_backward(xyz: torch.Tensor, grad_xyz: torch.Tensor, chain_idx: Optional[torch.Tensor] = None,
                                     residue_mask: Optional[torch.Tensor] = None, *, include_cb: bool = False,
                                     want_bond_angles: bool = False, want_bond_lengths: bool = False, out=None):
    """K12.  Vector-Jacobian product of ``backbone_from_dihedrals`` in one launch: from the coordinates ``xyz`` (B,N,A,3)
    that call returned (with the same ``chain_idx``, ``residue_mask``, ``include_cb``) and the upstream ``grad_xyz`` of
    the same shape, returns ``(grad_dihedrals, grad_bond_angles, grad_bond_lengths)``, each (B,N,3) fp32 in the
    forward's layout; the last two are None unless wanted (their arithmetic is skipped).  Entries the forward never
    reads are exact zeros; only slots 0, 1, 2 (and 4 with ``include_cb``) of unmasked rows are read, so NaN anywhere
    else never reaches the result; deterministic (include/protstruc_hip.h).  ``out``: a triple of contiguous fp32
    (B,N,3) tensors to write into (None where not wanted or to allocate); every element of them is written."""
    check_backbone_from_dihedrals_backward_shapes(xyz, grad_xyz, chain_idx, residue_mask, include_cb, want_bond_angles,
                                                  want_bond_lengths, out)
    xyz = _f32c(xyz, "xyz")
    outs = list(out) if out is not None else [None, None, None]
    _same_device(xyz, grad_xyz=grad_xyz, chain_idx=chain_idx, residue_mask=residue_mask,
                 **{f"out[{k}]": t for k, t in enumerate(outs)})
    gx, chain, rmask = _f32c(grad_xyz, "grad_xyz"), _f32c_opt(chain_idx, "chain_idx"), _u8c(residue_mask, "residue_mask")
    B, N, A = xyz.shape[:3]
    dev = xyz.device
    with _on(dev):
        for k, wanted in enumerate((True, want_bond_angles, want_bond_lengths)):
            if wanted and outs[k] is None:
                outs[k] = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
        if not (B == 0 or N == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_backbone_from_dihedrals_backward_f32", _ptr(xyz), _ptr(gx), _ptr(chain), _ptr(rmask),
                    _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), int(bool(include_cb)), B, N, A, _stream(xyz))
    return tuple(outs)



def check_distmat_shapes(d_cb, omega, theta, phi, mask=None, chain_breaks=None, lengths=None) -> None:
    """Shape rules of ``backbone_distmat_init`` on (B,L,L) inputs, on shapes only (no device, no launch): ValueError."""
    shape = tuple(d_cb.shape)
    if len(shape) != 3 or shape[1] != shape[2]:
        raise ValueError(f"d_cb must have shape (batch, L, L), got {shape}")
    for name, t, want in (("omega", omega, shape), ("theta", theta, shape), ("phi", phi, shape), ("mask", mask, shape),
                          ("chain_breaks", chain_breaks, shape[:2]), ("lengths", lengths, shape[:1])):
        _check_optional(t, want, name, "d_cb", shape)
    check_distmat_size(shape[0], shape[1])


def check_distmat_size(B: int, L: int) -> None:
    """The size limits of the K8 / K9 launches (a grid dimension per structure, 32-bit offsets in a structure)."""
    _check_batch(B)
    if 9 * L ** 2 >= 2 ** 31:
        raise ValueError(f"L = {L} is too long (9 L^2 must stay below 2^31)")


def _i32c(t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    _require_device(t, name)
    return t.to(torch.int32).contiguous()


def backbone_distmat_init(d_cb: torch.Tensor, omega: torch.Tensor, theta: torch.Tensor, phi: torch.Tensor,
                          mask: Optional[torch.Tensor] = None, chain_breaks: Optional[torch.Tensor] = None,
                          lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K8.  Steps 1-6 of the distance-matrix reconstruction: (B,L,L) d_cb / omega (trRosetta) / theta / phi, optional
    (B,L,L) pair ``mask``, (B,L) ``chain_breaks`` (chain ends after residue i) and (B,) ``lengths`` -> the (B,3,3,L,L)
    N / CA / C distance planes with MASK for unknown entries (include/protstruc_hip.h)."""
    check_distmat_shapes(d_cb, omega, theta, phi, mask, chain_breaks, lengths)
    d = _f32c(d_cb, "d_cb")
    _same_device(d, omega=omega, theta=theta, phi=phi, mask=mask, chain_breaks=chain_breaks, lengths=lengths)
    om, th, ph = _f32c(omega, "omega"), _f32c(theta, "theta"), _f32c(phi, "phi")
    m, brk, lens = _u8c(mask, "mask"), _u8c(chain_breaks, "chain_breaks"), _i32c(lengths, "lengths")
    B, L = d.shape[:2]
    dev = d.device
    with _on(dev):
        out = torch.empty(B, 3, 3, L, L, dtype=torch.float32, device=dev)
        if not (B == 0 or L == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_backbone_distmat_init_f32", _ptr(d), _ptr(om), _ptr(th), _ptr(ph), _ptr(m), _ptr(brk),
                    _ptr(lens), _ptr(out), B, L, _stream(d))
    return out


def check_floyd_warshall_shape(D, G: int = 1) -> Tuple[int, int]:
    """(B, L) of a Floyd-Warshall operand: (B,L,L) for G = 1, (B,G,G,L,L) for any G; ValueError otherwise."""
    shape = tuple(D.shape)
    if G < 1:
        raise ValueError(f"G must be >= 1, got {G}")
    if len(shape) == 5 and shape[1] == shape[2] == G and shape[3] == shape[4]:
        B, L = shape[0], shape[3]
    elif G == 1 and len(shape) == 3 and shape[1] == shape[2]:
        B, L = shape[0], shape[1]
    else:
        raise ValueError(f"D must have shape (batch, {G}, {G}, L, L)" + (" or (batch, L, L)" if G == 1 else "") +
                         f", got {shape}")
    _check_batch(B)
    if (G * L) ** 2 >= 2 ** 31:
        raise ValueError(f"{G * L} nodes are too many ((G L)^2 must stay below 2^31)")
    return B, L


def floyd_warshall_(D: torch.Tensor, G: int = 1) -> torch.Tensor:
    """K9.  All-pairs shortest paths in place, by the reference's rule D[r][c] = min(D[r][c], D[k][r] + D[k][c]) for
    k = 0 .. n-1 over the n = G L nodes (g, i) = g L + i of a contiguous float32 (B,G,G,L,L) tensor ((B,L,L) for G = 1).
    Bit for bit the sequential float32 loop when every entry is >= 0 and not NaN.  The workspace comes from torch's
    allocator on the current stream, so the call can be captured in a graph."""
    B, L = check_floyd_warshall_shape(D, G)
    _require_f32c(D, "D", "D must be a contiguous float32 tensor (it is updated in place)")
    lib = _lib.load()
    dev = D.device
    with _on(dev):
        if not (B == 0 or L == 0):
            nbytes = lib.ps_floyd_warshall_workspace_bytes(B, G, L)
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
            _launch("ps_floyd_warshall_f32", _ptr(D), B, G, L, _ptr(ws), nbytes, _stream(D))
    return D


def backbone_distmat_finish_(D: torch.Tensor, chain_breaks: Optional[torch.Tensor] = None,
                             lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Steps 8-9 in place on a (B,3,3,L,L) float32 tensor: (D + D^T) / 2 over the 3 L nodes, the bonds again (none
    across a chain break) and NaN for residues at or beyond ``lengths``."""
    B, L = check_floyd_warshall_shape(D, 3)
    _check_optional(chain_breaks, (B, L), "chain_breaks")
    _check_optional(lengths, (B,), "lengths")
    _require_f32c(D, "D", "D must be a contiguous float32 tensor (it is updated in place)")
    _same_device(D, chain_breaks=chain_breaks, lengths=lengths)
    brk, lens = _u8c(chain_breaks, "chain_breaks"), _i32c(lengths, "lengths")
    dev = D.device
    with _on(dev):
        if not (B == 0 or L == 0):
            _launch("ps_backbone_distmat_finish_f32", _ptr(D), _ptr(brk), _ptr(lens), B, L, _stream(D))
    return D


def check_lengths(lengths, B: int, L: int):
    """The ``lengths`` argument of a ragged batch of B structures of at most L residues, normalised: None, a (B,)
    tensor as it is (its shape is checked, its values stay where they are -- no copy to the host) or host integers
    as an int64 ndarray of B values in 0 .. L.  ValueError otherwise."""
    if lengths is None:
        return None
    if isinstance(lengths, (int, np.integer)):
        lengths = [int(lengths)]
    if not isinstance(lengths, torch.Tensor):
        lengths = np.asarray(lengths, dtype=np.int64)
    if tuple(lengths.shape) != (B,):
        raise ValueError(f"lengths must have shape ({B},), got {tuple(lengths.shape)}")
    if isinstance(lengths, np.ndarray) and ((lengths < 0).any() or (lengths > L).any()):
        raise ValueError(f"lengths must lie in 0 .. {L}, got {lengths.tolist()}")
    return lengths


def check_smacof_shapes(D, G: int = 1, n_init: Optional[int] = None, max_iter: int = 300, eps: float = 1e-6, init=None,
                        lengths=None) -> Tuple[int, int, int]:
    """Argument rules of ``smacof`` on shapes and values only (no device, no launch): (B, L, K) or ValueError."""
    B, L = check_floyd_warshall_shape(D, G)
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 1:
        raise ValueError(f"max_iter must be an integer >= 1, got {max_iter!r}")
    if not eps >= 0:
        raise ValueError(f"eps must be >= 0, got {eps!r}")
    if n_init is not None and (isinstance(n_init, bool) or not isinstance(n_init, int) or n_init < 1):
        raise ValueError(f"n_init must be an integer >= 1, got {n_init!r}")
    if init is not None:
        shape = tuple(init.shape)
        if len(shape) != 4 or shape[0] != B or shape[2] != G * L or shape[3] != 3:
            raise ValueError(f"init must have shape ({B}, n_init, {G * L}, 3), got {shape}")
        if n_init is not None and shape[1] != n_init:
            raise ValueError(f"init holds {shape[1]} starts, n_init = {n_init}")
        K = shape[1]
        if K < 1:
            raise ValueError("init must hold at least one start")
    else:
        K = 4 if n_init is None else n_init
    check_lengths(lengths, B, L)
    if K > MAX_BATCH or B * K * G * L * 3 >= 2 ** 31:
        raise ValueError(f"{B} x {K} starts of {G * L} nodes are too many for one call")
    return B, L, K


def _check_random_state(random_state):
    """sklearn.utils.check_random_state: None -> numpy's global RandomState, an int -> a new RandomState(seed), a
    RandomState -> itself."""
    if random_state is None or random_state is np.random:
        return np.random.mtrand._rand
    if isinstance(random_state, (int, np.integer)) and not isinstance(random_state, bool):
        return np.random.RandomState(random_state)
    if isinstance(random_state, np.random.RandomState):
        return random_state
    raise ValueError(f"{random_state!r} cannot be used to seed a numpy.random.RandomState instance")


def smacof_random_starts(B: int, K: int, G: int, L: int, lengths=None, random_state=None) -> np.ndarray:
    """sklearn's random SMACOF starts: for structure b = 0 .. B-1 and start k = 0 .. K-1 in turn,
    ``random_state.uniform(size=3 n)`` with n = G lengths[b], as (n, 3) rows, placed at nodes (g, i) = g L + i with
    i < lengths[b].  Returns (B, K, G L, 3) float64 (0 at padded nodes); host work only."""
    rs = _check_random_state(random_state)
    out = np.zeros((B, K, G, L, 3), dtype=np.float64)
    for b in range(B):
        ln = L if lengths is None else int(lengths[b])
        for k in range(K):
            out[b, k, :, :ln] = rs.uniform(size=3 * G * ln).reshape(G, ln, 3)
    return out.reshape(B, K, G * L, 3)


def smacof(D: torch.Tensor, G: int = 1, *, n_init: Optional[int] = None, max_iter: int = 300, eps: float = 1e-6,
           init: Optional[torch.Tensor] = None, random_state=None, lengths=None):
    """K10.  Metric SMACOF (sklearn 1.7's ``smacof``) on the n = G L nodes (g, i) = g L + i of a float32 (B,G,G,L,L)
    dissimilarity tensor ((B,L,L) for G = 1) on the GPU: returns (X (B, G L, 3) float32, stress (B,) float64, n_iter (B,)
    int32) of the best of K starts (include/protstruc_hip.h).

    Starts: ``init`` (B, K, G L, 3) on D's device -- K explicit starts, an extension (sklearn runs one start when given
    ``init``) -- or K = ``n_init`` (default 4) random ones drawn on the host exactly as sklearn draws them from
    ``random_state`` (None: numpy's global state; see ``smacof_random_starts``).  ``lengths`` (B,) restricts structure
    b to the nodes i < lengths[b]; padded rows of X are NaN.  Without ``random_state`` draws the call is capturable."""
    B, L, K = check_smacof_shapes(D, G, n_init, max_iter, eps, init, lengths)
    lengths = check_lengths(lengths, B, L)
    if random_state is not None and init is not None:
        raise ValueError("random_state draws starts; it cannot be combined with an explicit init")
    _require_device(D, "D")
    dev = D.device
    d = _f32c(D, "D")
    if init is None:
        # the random starts are drawn on the host, per structure length: a tensor's values are fetched (and checked)
        lens_host = check_lengths(lengths.cpu().numpy(), B, L) if isinstance(lengths, torch.Tensor) else lengths
        starts = smacof_random_starts(B, K, G, L, lens_host, random_state)
        x0 = torch.from_numpy(starts.astype(np.float32)).to(dev)
    else:
        _same_device(d, init=init)
        x0 = _f32c(init, "init")
    if lengths is not None:
        lens = _i32c(lengths if isinstance(lengths, torch.Tensor) else torch.from_numpy(lengths).to(dev), "lengths")
        _same_device(d, lengths=lens)
    else:
        lens = None
    lib = _lib.load()
    with _on(dev):
        X = torch.empty(B, G * L, 3, dtype=torch.float32, device=dev)
        stress = torch.empty(B, dtype=torch.float64, device=dev)
        n_iter = torch.empty(B, dtype=torch.int32, device=dev)
        if B > 0:
            nbytes = lib.ps_smacof_workspace_bytes(B, K, G, L)
            ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
            _launch("ps_smacof_f32", _ptr(d), B, G, L, _ptr(lens), _ptr(x0), K, max_iter, float(eps), _ptr(X),
                    _ptr(stress), _ptr(n_iter), _ptr(ws), ws.numel() * 8, _stream(d))
    return X, stress, n_iter


def check_backbone_coords_shape(X, n_atoms: int = 3) -> Tuple[int, int]:
    """(B, L) of (B, n_atoms, L, 3) backbone coordinates; ValueError otherwise."""
    shape = tuple(X.shape)
    if len(shape) != 4 or shape[1] != n_atoms or shape[3] != 3:
        raise ValueError(f"coordinates must have shape (batch, {n_atoms}, L, 3), got {shape}")
    _check_batch(shape[0])
    return shape[0], shape[2]


def mds_backbone_finish(X: torch.Tensor, lengths: Optional[torch.Tensor] = None, *, mirror: bool = True,
                        place_o_cb: bool = True) -> torch.Tensor:
    """K11.  (B,3,L,3) N / CA / C coordinates (an MDS result reshaped) -> (B,5,L,3) N, CA, C, O, CB (``place_o_cb``) or
    (B,3,L,3) N, CA, C.  With ``mirror`` z is negated where the mean backbone phi is positive (the hand a protein does
    not have); ``mirror=False`` never mirrors.  O of the last residue is placed from N of the first (the reference's
    np.roll).  Padded residues (``lengths``) are NaN; a NaN in a structure makes its whole output NaN."""
    B, L = check_backbone_coords_shape(X, 3)
    lengths = check_lengths(lengths, B, L)
    x = _f32c(X, "X")
    _same_device(x, lengths=lengths)
    lens = _i32c(lengths, "lengths")
    A = 5 if place_o_cb else 3
    dev = x.device
    with _on(dev):
        out = torch.empty(B, A, L, 3, dtype=torch.float32, device=dev)
        if not (B == 0 or L == 0):
            _launch("ps_mds_backbone_finish_f32", _ptr(x), _ptr(lens), B, L, 1 if mirror else 0, A, _ptr(out),
                    _stream(x))
    return out


def frames(xyz: torch.Tensor, a1: int, a2: int, a3: int, t_atom: int = 1, *, want_rot: bool = True,
           want_trans: bool = True):
    """K4.  Returns (rot (B,N,3,3) or None, trans (B,N,3) or None)."""
    xyz = _f32c(xyz, "xyz")
    B, N, A = xyz.shape[:3]
    dev = xyz.device
    with _on(dev):
        rot = torch.empty(B, N, 3, 3, dtype=torch.float32, device=dev) if want_rot else None
        trans = torch.empty(B, N, 3, dtype=torch.float32, device=dev) if want_trans else None
        if not (B == 0 or N == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_frames_f32", _ptr(xyz), _ptr(rot), _ptr(trans), B, N, A, int(a1), int(a2), int(a3), int(t_atom),
                    _stream(xyz))
    return rot, trans


def check_frames_backward_shapes(xyz, a1: int, a2: int, a3: int, t_atom: int = 1, grad_rot=None, grad_trans=None,
                                 residue_mask=None, out=None) -> None:
    """Shape rules of ``frames_backward``, on shapes, dtypes and slots only (no device, no launch): ValueError."""
    B, N, A = _xyz_dims(xyz)
    shape = (B, N, A, 3)
    if grad_rot is None and grad_trans is None:
        raise ValueError("at least one of grad_rot and grad_trans is required")
    like = f"xyz {shape}"
    if grad_rot is not None:
        _check_float_tensor(grad_rot, (B, N, 3, 3), "grad_rot", like)
        _check_atom_slots(A, a1, a2, a3)
    if grad_trans is not None:
        _check_float_tensor(grad_trans, (B, N, 3), "grad_trans", like)
        _check_atom_slots(A, t_atom)
    _check_optional(residue_mask, (B, N), "residue_mask", "xyz", shape)
    _check_out(out, shape, "out")


def frames_backward(xyz: torch.Tensor, a1: int, a2: int, a3: int, t_atom: int = 1, *,
                    grad_rot: Optional[torch.Tensor] = None, grad_trans: Optional[torch.Tensor] = None,
                    residue_mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Vector-Jacobian product of K4 (``frames``) in one launch: ``grad_xyz`` (B,N,A,3) fp32 from the upstream
    ``grad_rot`` (B,N,3,3; any 3x3, not assumed tangent to the rotations) and / or ``grad_trans`` (B,N,3); an absent one
    is zero and its arithmetic is skipped.  Contributions are summed where slots coincide; every element of the result is
    written: slots that are not read, and residues absent from ``residue_mask`` (B,N), are exact zeros -- NaN there never
    reaches the result (include/protstruc_hip.h)."""
    check_frames_backward_shapes(xyz, a1, a2, a3, t_atom, grad_rot, grad_trans, residue_mask, out)
    xyz = _f32c(xyz, "xyz")
    _same_device(xyz, grad_rot=grad_rot, grad_trans=grad_trans, residue_mask=residue_mask, out=out)
    g_rot, g_trans = _f32c_opt(grad_rot, "grad_rot"), _f32c_opt(grad_trans, "grad_trans")
    rmask = _u8c(residue_mask, "residue_mask")
    B, N, A = xyz.shape[:3]
    with _on(xyz.device):
        if out is None:
            out = torch.empty(B, N, A, 3, dtype=torch.float32, device=xyz.device)
        if not (B == 0 or N == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_frames_backward_f32", _ptr(xyz), _ptr(g_rot), _ptr(g_trans), _ptr(rmask), _ptr(out), B, N, A,
                    int(a1), int(a2), int(a3), int(t_atom), _stream(xyz))
    return out


FAPE_FRAME_TILE = 64   # PS_FAPE_FRAME_TILE of include/protstruc_hip.h: frames per workgroup = one partial sum each


def check_fape_shapes(rot, trans, points, target_rot, target_trans, target_points, frame_mask=None, point_mask=None,
                      clamp=10.0, scale=10.0, eps=1e-4, grad_loss=None) -> None:
    """Shape rules of ``fape`` / ``fape_backward``, on shapes, dtypes, devices and the three scalars only (no launch):
    ValueError.  ``clamp`` is a positive float (``inf`` = unclamped) or a (B,) float tensor; the values of a tensor are
    checked where that costs no device synchronisation, i.e. when it lives on the host."""
    shape = tuple(rot.shape)
    if len(shape) != 4 or shape[2:] != (3, 3):
        raise ValueError(f"rot must have shape (batch, frames, 3, 3), got {shape}")
    B, N = shape[:2]
    pshape = tuple(points.shape)
    if len(pshape) != 3 or pshape[0] != B or pshape[2] != 3:
        raise ValueError(f"points must have shape ({B}, points, 3), got {pshape}")
    M = pshape[1]
    _check_batch(B)
    if N > 2 ** 30 or M > 2 ** 30:
        raise ValueError(f"at most 2^30 frames and points per structure, got {N} and {M}")
    like = f"rot {shape} and points {pshape}"
    for name, t, want in (("rot", rot, shape), ("trans", trans, (B, N, 3)), ("points", points, pshape),
                          ("target_rot", target_rot, shape), ("target_trans", target_trans, (B, N, 3)),
                          ("target_points", target_points, pshape)):
        _check_float_tensor(t, want, name, like)
    _check_optional(frame_mask, (B, N), "frame_mask")
    _check_optional(point_mask, (B, M), "point_mask")
    if isinstance(clamp, torch.Tensor):
        _check_float_tensor(clamp, (B,), "clamp", f"rot {shape}")
        if not clamp.is_cuda and not bool((clamp > 0).all()):
            raise ValueError("clamp must be positive (inf = unclamped)")
    elif not float(clamp) > 0:
        raise ValueError(f"clamp must be positive (inf = unclamped), got {clamp}")
    _check_scalar(scale, "scale", "positive")
    _check_scalar(eps, "eps", "non-negative")
    if grad_loss is not None:
        _check_float_tensor(grad_loss, (B,), "grad_loss", f"rot {shape}")
    tensors = {"trans": trans, "points": points, "target_rot": target_rot, "target_trans": target_trans,
               "target_points": target_points, "frame_mask": frame_mask, "point_mask": point_mask, "grad_loss": grad_loss}
    if isinstance(clamp, torch.Tensor):
        tensors["clamp"] = clamp
    _same_device(rot, **tensors)


def _fape_operands(rot, trans, points, target_rot, target_trans, target_points, frame_mask, point_mask, clamp):
    """The eight tensor operands of the two FAPE launches as the kernels read them, and the (B,) clamp on the device."""
    rot = _f32c(rot, "rot")
    floats = [rot] + [_f32c(t, name) for t, name in ((trans, "trans"), (points, "points"), (target_rot, "target_rot"),
                                                      (target_trans, "target_trans"), (target_points, "target_points"))]
    if isinstance(clamp, torch.Tensor):
        clamp = _f32c(clamp, "clamp")
    else:
        clamp = torch.full((rot.shape[0],), float(clamp), dtype=torch.float32, device=rot.device)
    return floats, _u8c(frame_mask, "frame_mask"), _u8c(point_mask, "point_mask"), clamp


def fape(rot: torch.Tensor, trans: torch.Tensor, points: torch.Tensor, target_rot: torch.Tensor,
         target_trans: torch.Tensor, target_points: torch.Tensor, frame_mask: Optional[torch.Tensor] = None,
         point_mask: Optional[torch.Tensor] = None, *, clamp=10.0, scale: float = 10.0, eps: float = 1e-4):
    """K13.  Frame-aligned point error, fused: ``(loss (B,), count (B,))`` fp32 with
    ``loss[b] = mean over valid (frame i, point j) of min(sqrt(|R_i^T (x_j - t_i) - R'_i^T (x'_j - t'_i)|^2 + eps), clamp[b]) / scale``
    and ``count[b]`` the number of valid pairs (``frame_mask`` (B,N) times ``point_mask`` (B,M); None = all), as fp32:
    exact below 2^24 pairs per structure, rounded above.  ``rot``
    (B,N,3,3) has the basis vectors as columns, as ``frames`` returns it; ``points`` (B,M,3) may be the (B, N*A, 3) view
    of coordinates with the atom mask as ``point_mask`` (masked points cost nothing).  ``clamp``: a float or a (B,)
    tensor, ``inf`` = unclamped.  A structure without a valid pair has loss 0; NaN at masked frames / points never
    reaches the result; deterministic (include/protstruc_hip.h)."""
    check_fape_shapes(rot, trans, points, target_rot, target_trans, target_points, frame_mask, point_mask, clamp, scale, eps)
    floats, fm, pm, cl = _fape_operands(rot, trans, points, target_rot, target_trans, target_points, frame_mask,
                                        point_mask, clamp)
    B, N, M = floats[0].shape[0], floats[0].shape[1], floats[2].shape[1]
    dev = floats[0].device
    with _on(dev):
        if B == 0 or N == 0 or M == 0:   # empty input: nothing to launch (an empty tensor has no device pointer); no pair
            return torch.zeros(B, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.float32, device=dev)
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        count = torch.empty(B, dtype=torch.float32, device=dev)
        partials = torch.empty(B * -(-N // FAPE_FRAME_TILE), dtype=torch.float64, device=dev)   # one sum per workgroup
        _launch("ps_fape_f32", *[_ptr(t) for t in floats], _ptr(fm), _ptr(pm), _ptr(cl), float(scale), float(eps),
                _ptr(loss), _ptr(count), _ptr(partials), B, N, M, _stream(loss))
    return loss, count


def fape_backward(rot: torch.Tensor, trans: torch.Tensor, points: torch.Tensor, target_rot: torch.Tensor,
                  target_trans: torch.Tensor, target_points: torch.Tensor, grad_loss: torch.Tensor,
                  frame_mask: Optional[torch.Tensor] = None, point_mask: Optional[torch.Tensor] = None, *, clamp=10.0,
                  scale: float = 10.0, eps: float = 1e-4, want_rot: bool = True, want_trans: bool = True,
                  want_points: bool = True):
    """K14.  Vector-Jacobian product of ``fape`` with respect to the predicted side in one launch that recomputes the
    pairs: ``(grad_rot (B,N,3,3), grad_trans (B,N,3), grad_points (B,M,3))`` fp32 from the upstream ``grad_loss`` (B,).
    A gradient that is not wanted comes back as None and its work is skipped (the frame-owned workgroups compute
    ``grad_rot`` and ``grad_trans`` together, the point-owned ones ``grad_points``).  ``grad_rot`` is the unconstrained
    3x3 gradient.  A pair passes gradient iff its distance is below ``clamp``; masked frames and points get exact zeros
    and NaN there never reaches an output; the target side gets no gradient; deterministic (include/protstruc_hip.h).
    With ``eps = 0`` a valid pair whose two sides coincide has distance 0 and no derivative: its rows come out NaN, as under
    autograd, so keep ``eps > 0`` where prediction and target can be equal."""
    check_fape_shapes(rot, trans, points, target_rot, target_trans, target_points, frame_mask, point_mask, clamp, scale,
                      eps, grad_loss)
    if not (want_rot or want_trans or want_points):
        raise ValueError("at least one gradient must be wanted")
    floats, fm, pm, cl = _fape_operands(rot, trans, points, target_rot, target_trans, target_points, frame_mask,
                                        point_mask, clamp)
    g = _f32c(grad_loss, "grad_loss")
    B, N, M = floats[0].shape[0], floats[0].shape[1], floats[2].shape[1]
    dev = floats[0].device
    with _on(dev):
        # empty input: nothing to launch (an empty tensor has no device pointer); without a pair every gradient is zero
        alloc = torch.zeros if (B == 0 or N == 0 or M == 0) else torch.empty
        g_rot = alloc(B, N, 3, 3, dtype=torch.float32, device=dev) if want_rot else None
        g_trans = alloc(B, N, 3, dtype=torch.float32, device=dev) if want_trans else None
        g_pts = alloc(B, M, 3, dtype=torch.float32, device=dev) if want_points else None
        if alloc is torch.empty:
            _launch("ps_fape_backward_f32", *[_ptr(t) for t in floats], _ptr(fm), _ptr(pm), _ptr(cl), float(scale),
                    float(eps), _ptr(g), _ptr(g_rot), _ptr(g_trans), _ptr(g_pts), B, N, M, _stream(g))
    return g_rot, g_trans, g_pts


LDDT_THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
LDDT_MAX_THRESHOLDS = 8     # PS_LDDT_MAX_THRESHOLDS of include/protstruc_hip.h
LDDT_MAX_THRESHOLD = 64.0   # PS_LDDT_MAX_THRESHOLD: exp(-threshold) stays a normal float32


def check_lddt_shapes(points, target_points, point_mask=None, groups=None, cutoff=15.0, thresholds=LDDT_THRESHOLDS,
                      eps=1e-10, grad_S=None) -> None:
    """Shape rules of ``lddt`` / ``lddt_backward``, on shapes, dtypes, devices and the scalars only (no launch):
    ValueError.  ``thresholds``: 1 to 8 strictly increasing floats in (0, 64]; ``cutoff`` positive and finite; ``groups``
    an integer tensor."""
    B, M = _points_dims(points, 2 ** 30)
    like = f"points {(B, M, 3)}"
    _check_float_tensor(target_points, (B, M, 3), "target_points", like)
    _check_optional(point_mask, (B, M), "point_mask")
    _check_optional(groups, (B, M), "groups", integer=True)
    _check_scalar(cutoff, "cutoff", "positive")
    thr = [float(t) for t in thresholds]
    if not 1 <= len(thr) <= LDDT_MAX_THRESHOLDS:
        raise ValueError(f"between 1 and {LDDT_MAX_THRESHOLDS} thresholds, got {len(thr)}")
    if not all(0 < t <= LDDT_MAX_THRESHOLD for t in thr) or any(b <= a for a, b in zip(thr, thr[1:])):
        raise ValueError(f"thresholds must be strictly increasing and in (0, {LDDT_MAX_THRESHOLD}], got {tuple(thr)}")
    _check_scalar(eps, "eps", "non-negative")
    if grad_S is not None:
        _check_float_tensor(grad_S, (B, M), "grad_S", like)
    _same_device(points, target_points=target_points, point_mask=point_mask, groups=groups, grad_S=grad_S)


def _lddt_operands(points, target_points, point_mask, groups, thresholds):
    thr = (ctypes.c_float * len(thresholds))(*[float(t) for t in thresholds])   # a host array: the library reads it there
    return (_f32c(points, "points"), _f32c(target_points, "target_points"), _u8c(point_mask, "point_mask"),
            _i32c(groups, "groups"), thr)


def lddt(points: torch.Tensor, target_points: torch.Tensor, point_mask: Optional[torch.Tensor] = None,
         groups: Optional[torch.Tensor] = None, *, cutoff: float = 15.0, thresholds=LDDT_THRESHOLDS, smooth: bool = False,
         eps: float = 1e-10):
    """K15.  lDDT per point, fused: ``(S (B,M), n (B,M))`` fp32 with ``n_i`` the number of points j that count for point
    i -- both in ``point_mask`` (None = all), ``j != i``, in another group where ``groups`` (B,M; integers) are given, and
    within ``cutoff`` of i ON THE TARGET -- and ``S_i`` the sum over them of the fraction of ``thresholds`` that
    ``| |x_i - x_j| - |x'_i - x'_j| |`` stays under (``smooth=False``, the metric), or of the mean of
    ``sigmoid(threshold - that difference)`` (``smooth=True``, AlphaFold 3 suppl. alg. 27).  The score of a point is
    ``S / n.clamp(min=1)``; a point without a partner has ``S = n = 0``.  Distances are ``sqrt(|.|^2 + eps)``.  ``points``
    may be the (B, N*A, 3) view of coordinates with the atom mask as ``point_mask`` and the residue index as ``groups``.
    Nothing of size M^2 is built; masked points get zeros and NaN there never reaches the result; deterministic
    (include/protstruc_hip.h)."""
    check_lddt_shapes(points, target_points, point_mask, groups, cutoff, thresholds, eps)
    x, t, pm, gr, thr = _lddt_operands(points, target_points, point_mask, groups, thresholds)
    B, M = x.shape[:2]
    with _on(x.device):
        if B == 0 or M == 0:   # empty input: nothing to launch (an empty tensor has no device pointer)
            return torch.zeros(B, M, dtype=torch.float32, device=x.device), torch.zeros(B, M, dtype=torch.float32, device=x.device)
        S = torch.empty(B, M, dtype=torch.float32, device=x.device)
        n = torch.empty(B, M, dtype=torch.float32, device=x.device)
        _launch("ps_lddt_f32", _ptr(x), _ptr(t), _ptr(pm), _ptr(gr), float(cutoff), thr, len(thr), int(bool(smooth)),
                float(eps), _ptr(S), _ptr(n), B, M, _stream(x))
    return S, n


def lddt_backward(points: torch.Tensor, target_points: torch.Tensor, grad_S: torch.Tensor,
                  point_mask: Optional[torch.Tensor] = None, groups: Optional[torch.Tensor] = None, *,
                  cutoff: float = 15.0, thresholds=LDDT_THRESHOLDS, eps: float = 1e-10) -> torch.Tensor:
    """K16.  Vector-Jacobian product of ``lddt(..., smooth=True)`` with respect to ``points`` in one launch that
    recomputes the pairs: ``grad_points`` (B,M,3) fp32 from the upstream ``grad_S`` (B,M).  Every element is written;
    masked points get exact zeros and NaN there never reaches the result; a prediction equal to its target has an exactly
    zero gradient; the target gets no gradient; deterministic (include/protstruc_hip.h).  Keep ``eps > 0``: with
    ``eps = 0`` two coincident predicted points that count for each other have no derivative (NaN, as under autograd)."""
    check_lddt_shapes(points, target_points, point_mask, groups, cutoff, thresholds, eps, grad_S)
    x, t, pm, gr, thr = _lddt_operands(points, target_points, point_mask, groups, thresholds)
    g = _f32c(grad_S, "grad_S")
    B, M = x.shape[:2]
    with _on(x.device):
        if B == 0 or M == 0:
            return torch.zeros(B, M, 3, dtype=torch.float32, device=x.device)
        out = torch.empty(B, M, 3, dtype=torch.float32, device=x.device)
        _launch("ps_lddt_backward_f32", _ptr(x), _ptr(t), _ptr(pm), _ptr(gr), float(cutoff), thr, len(thr), float(eps),
                _ptr(g), _ptr(out), B, M, _stream(x))
    return out


VDW_RADII = {"C": 1.7, "N": 1.55, "O": 1.52, "S": 1.8}   # van der Waals radii by element (AlphaFold 2 suppl. 1.9.11)
CLASH_TOLERANCE = 1.5
# ideal peptide-bond geometry and its standard deviations (AlphaFold 2 suppl. 1.9.11; Engh & Huber 2001), and the
# tolerance factor tau: a deviation of up to tau standard deviations is no violation
PEPTIDE_BOND = dict(l0=1.329, sigma_l=0.014, l0_pro=1.341, sigma_l_pro=0.016, cos_cacn=-0.4473, sigma_cacn=0.0311,
                    cos_cnca=-0.5203, sigma_cnca=0.0353, tau=12.0)
PEPTIDE_BOND_CONSTANTS = 12   # PS_PEPTIDE_BOND_CONSTANTS of include/protstruc_hip.h


def check_clash_shapes(points, radius, point_mask=None, groups=None, link=None, tolerance=CLASH_TOLERANCE, eps=1e-10,
                       grad_E=None) -> None:
    """Shape rules of ``clash`` / ``clash_backward``, on shapes, dtypes, devices and the scalars only (no launch):
    ValueError.  ``groups`` and ``link`` are integer tensors; ``tolerance`` finite; ``eps`` non-negative and finite."""
    B, M = _points_dims(points, 2 ** 30)
    like = f"points {(B, M, 3)}"
    _check_float_tensor(radius, (B, M), "radius", like)
    _check_optional(point_mask, (B, M), "point_mask")
    _check_optional(groups, (B, M), "groups", integer=True)
    _check_optional(link, (B, M), "link", integer=True)
    _check_scalar(tolerance, "tolerance", "finite")
    _check_scalar(eps, "eps", "non-negative")
    if grad_E is not None:
        _check_float_tensor(grad_E, (B, M), "grad_E", like)
    _same_device(points, radius=radius, point_mask=point_mask, groups=groups, link=link, grad_E=grad_E)


def _clash_operands(points, radius, point_mask, groups, link):
    return (_f32c(points, "points"), _f32c(radius, "radius"), _u8c(point_mask, "point_mask"), _i32c(groups, "groups"),
            _i32c(link, "link"))


def clash(points: torch.Tensor, radius: torch.Tensor, point_mask: Optional[torch.Tensor] = None,
          groups: Optional[torch.Tensor] = None, link: Optional[torch.Tensor] = None, *,
          tolerance: float = CLASH_TOLERANCE, eps: float = 1e-10):
    """K17.  Steric clash energy per point, fused: ``(E (B,M), n (B,M))`` fp32 with ``E_i`` the sum over the points j
    that count for point i -- both in ``point_mask`` (None = all), ``j != i``, in another group where ``groups`` (B,M;
    integers) are given, and not carrying the same non-negative ``link`` (B,M; integers: a covalent bond between groups)
    -- of ``max(0, radius_i + radius_j - tolerance - sqrt(|x_i - x_j|^2 + eps))``, and ``n_i`` the number of them that
    overlap.  Every clashing pair appears in both owners' sums.  ``points`` may be the (B, N*A, 3) view of coordinates
    with the atom mask as ``point_mask`` and the residue index as ``groups``.  Nothing of size M^2 is built; masked
    points get zeros and NaN there (coordinates or radii) never reaches the result; deterministic
    (include/protstruc_hip.h)."""
    check_clash_shapes(points, radius, point_mask, groups, link, tolerance, eps)
    x, r, pm, gr, lk = _clash_operands(points, radius, point_mask, groups, link)
    B, M = x.shape[:2]
    with _on(x.device):
        if B == 0 or M == 0:   # empty input: nothing to launch (an empty tensor has no device pointer)
            return torch.zeros(B, M, dtype=torch.float32, device=x.device), torch.zeros(B, M, dtype=torch.float32, device=x.device)
        E = torch.empty(B, M, dtype=torch.float32, device=x.device)
        n = torch.empty(B, M, dtype=torch.float32, device=x.device)
        _launch("ps_clash_f32", _ptr(x), _ptr(r), _ptr(pm), _ptr(gr), _ptr(lk), float(tolerance), float(eps), _ptr(E),
                _ptr(n), B, M, _stream(x))
    return E, n


def clash_backward(points: torch.Tensor, radius: torch.Tensor, grad_E: torch.Tensor,
                   point_mask: Optional[torch.Tensor] = None, groups: Optional[torch.Tensor] = None,
                   link: Optional[torch.Tensor] = None, *, tolerance: float = CLASH_TOLERANCE,
                   eps: float = 1e-10) -> torch.Tensor:
    """K18.  Vector-Jacobian product of ``clash`` with respect to ``points`` in one launch that recomputes the pairs:
    ``grad_points`` (B,M,3) fp32 from the upstream ``grad_E`` (B,M).  Every element is written; masked points get exact
    zeros and NaN there never reaches the result; the radii get no gradient; deterministic (include/protstruc_hip.h).
    Keep ``eps > 0``: with ``eps = 0`` two coincident points that count for each other have no derivative (NaN, as under
    autograd)."""
    check_clash_shapes(points, radius, point_mask, groups, link, tolerance, eps, grad_E)
    x, r, pm, gr, lk = _clash_operands(points, radius, point_mask, groups, link)
    g = _f32c(grad_E, "grad_E")
    B, M = x.shape[:2]
    with _on(x.device):
        if B == 0 or M == 0:
            return torch.zeros(B, M, 3, dtype=torch.float32, device=x.device)
        out = torch.empty(B, M, 3, dtype=torch.float32, device=x.device)
        _launch("ps_clash_backward_f32", _ptr(x), _ptr(r), _ptr(pm), _ptr(gr), _ptr(lk), float(tolerance), float(eps),
                _ptr(g), _ptr(out), B, M, _stream(x))
    return out


def _peptide_bond_constants(eps, constants):
    """The twelve floats of the C ABI from ``PEPTIDE_BOND`` overridden by ``constants``; ValueError for an unknown name,
    a value that is not finite, or a negative sigma, tau or eps."""
    unknown = set(constants) - set(PEPTIDE_BOND)
    if unknown:
        raise ValueError(f"unknown peptide-bond constants {sorted(unknown)}; the names are {sorted(PEPTIDE_BOND)}")
    k = {name: float(value) for name, value in {**PEPTIDE_BOND, **constants}.items()}
    k["eps"] = float(eps)
    for name, value in k.items():
        if not abs(value) < float("inf"):
            raise ValueError(f"{name} must be finite, got {value}")
        if (name.startswith("sigma") or name in ("tau", "eps")) and value < 0:
            raise ValueError(f"{name} must be non-negative, got {value}")
    order = ("l0", "sigma_l", "l0_pro", "sigma_l_pro", "cos_cacn", "sigma_cacn", "cos_cnca", "sigma_cnca", "tau", "eps")
    return [k[name] for name in order] + [0.0] * (PEPTIDE_BOND_CONSTANTS - len(order))


def check_peptide_bond_shapes(xyz, junction_mask=None, next_is_proline=None, n_slot: int = 0, ca_slot: int = 1,
                              c_slot: int = 2, eps=1e-10, grad_viol=None, **constants) -> None:
    """Shape rules of ``peptide_bond`` / ``peptide_bond_backward``, on shapes, dtypes, devices, slots and the constants
    only (no launch): ValueError.  The three slots differ; ``constants`` are names of ``PEPTIDE_BOND``."""
    B, N, A = _xyz_dims(xyz)
    shape = (B, N, A, 3)
    if B * N > 2 ** 31:
        raise ValueError(f"at most 2^31 residues per call, got {B * N}")
    _check_atom_slots(A, n_slot, ca_slot, c_slot)
    if len({int(n_slot), int(ca_slot), int(c_slot)}) != 3:
        raise ValueError(f"the N, CA and C slots must differ, got {(n_slot, ca_slot, c_slot)}")
    _check_optional(junction_mask, (B, N), "junction_mask", "xyz", shape)
    _check_optional(next_is_proline, (B, N), "next_is_proline", "xyz", shape)
    _peptide_bond_constants(eps, constants)
    if grad_viol is not None:
        _check_float_tensor(grad_viol, (B, N, 3), "grad_viol", f"xyz {shape}")
    _same_device(xyz, junction_mask=junction_mask, next_is_proline=next_is_proline, grad_viol=grad_viol)


def peptide_bond(xyz: torch.Tensor, junction_mask: Optional[torch.Tensor] = None,
                 next_is_proline: Optional[torch.Tensor] = None, *, n_slot: int = 0, ca_slot: int = 1, c_slot: int = 2,
                 eps: float = 1e-10, **constants) -> torch.Tensor:
    """K19.  Peptide-bond violations at every junction r -> r+1: ``viol`` (B,N,3) fp32 = how far the bond length
    |C - N'|, the cosine of the angle CA-C-N' and the cosine of the angle C-N'-CA' lie outside ``tau`` standard deviations
    around their ideal values (``PEPTIDE_BOND``; any of its names may be overridden by keyword).  ``junction_mask`` (B,N):
    entry r is the junction from residue r to r+1 (None = all valid; entry N-1 is ignored); ``next_is_proline`` (B,N):
    residue r+1 is a proline, which has its own ideal bond length (None = none).  Invalid junctions and row N-1 get exact
    zeros, whatever NaN sits there (include/protstruc_hip.h)."""
    check_peptide_bond_shapes(xyz, junction_mask, next_is_proline, n_slot, ca_slot, c_slot, eps, **constants)
    k = (ctypes.c_float * PEPTIDE_BOND_CONSTANTS)(*_peptide_bond_constants(eps, constants))   # a host array
    x, jm, pro = _f32c(xyz, "xyz"), _u8c(junction_mask, "junction_mask"), _u8c(next_is_proline, "next_is_proline")
    B, N, A = x.shape[:3]
    with _on(x.device):
        if B == 0 or N == 0:   # empty input: nothing to launch (an empty tensor has no device pointer)
            return torch.zeros(B, N, 3, dtype=torch.float32, device=x.device)
        viol = torch.empty(B, N, 3, dtype=torch.float32, device=x.device)
        _launch("ps_peptide_bond_f32", _ptr(x), _ptr(jm), _ptr(pro), int(n_slot), int(ca_slot), int(c_slot), k, _ptr(viol),
                B, N, A, _stream(x))
    return viol


def peptide_bond_backward(xyz: torch.Tensor, grad_viol: torch.Tensor, junction_mask: Optional[torch.Tensor] = None,
                          next_is_proline: Optional[torch.Tensor] = None, *, n_slot: int = 0, ca_slot: int = 1,
                          c_slot: int = 2, eps: float = 1e-10, **constants) -> torch.Tensor:
    """K20.  Vector-Jacobian product of ``peptide_bond`` in one launch: ``grad_xyz`` (B,N,A,3) fp32 from the upstream
    ``grad_viol`` (B,N,3).  Every element is written: slots other than N, CA and C, and the atoms of invalid junctions,
    are exact zeros, and neither coordinates nor ``grad_viol`` are read at an invalid junction; no atomics, deterministic
    (include/protstruc_hip.h)."""
    check_peptide_bond_shapes(xyz, junction_mask, next_is_proline, n_slot, ca_slot, c_slot, eps, grad_viol, **constants)
    k = (ctypes.c_float * PEPTIDE_BOND_CONSTANTS)(*_peptide_bond_constants(eps, constants))
    x, jm, pro = _f32c(xyz, "xyz"), _u8c(junction_mask, "junction_mask"), _u8c(next_is_proline, "next_is_proline")
    g = _f32c(grad_viol, "grad_viol")
    B, N, A = x.shape[:3]
    with _on(x.device):
        if B == 0 or N == 0:
            return torch.zeros(B, N, A, 3, dtype=torch.float32, device=x.device)
        out = torch.empty(B, N, A, 3, dtype=torch.float32, device=x.device)
        _launch("ps_peptide_bond_backward_f32", _ptr(x), _ptr(jm), _ptr(pro), int(n_slot), int(ca_slot), int(c_slot), k,
                _ptr(g), _ptr(out), B, N, A, _stream(x))
    return out


DSSP_MAX_RESIDUES = 2048   # PS_DSSP_MAX_RESIDUES of include/protstruc_hip.h: the assignment keeps a structure's lists in LDS


def check_dssp_shapes(xyz, complete, junction, donor=None, n_slot: int = 0, ca_slot: int = 1, c_slot: int = 2,
                      o_slot: int = 3, acceptor_idx=None) -> None:
    """Shape rules of ``backbone_hbonds`` / ``dssp_assign``, on shapes, dtypes, devices and slots only (no launch):
    ValueError.  The four slots differ; with ``acceptor_idx`` (the assignment) only ``ca_slot`` counts and a structure
    has at most ``DSSP_MAX_RESIDUES`` residues."""
    B, N, A = _xyz_dims(xyz)
    shape = (B, N, A, 3)
    _check_batch(B)
    _check_count(N, 0, 2 ** 24, "residues per structure")
    if acceptor_idx is None:
        if A < 4:
            raise ValueError(f"xyz needs slots for N, CA, C and O, got {A} atoms per residue")
        _check_atom_slots(A, n_slot, ca_slot, c_slot, o_slot)
        if len({int(n_slot), int(ca_slot), int(c_slot), int(o_slot)}) != 4:
            raise ValueError(f"the N, CA, C and O slots must differ, got {(n_slot, ca_slot, c_slot, o_slot)}")
    else:
        _check_atom_slots(A, ca_slot)
    for name, t in (("complete", complete), ("junction", junction), ("donor", donor)):
        if t is None and name != "donor":
            raise ValueError(f"{name} is required")
        _check_optional(t, (B, N), name, "xyz", shape)
    if acceptor_idx is not None:
        if N > DSSP_MAX_RESIDUES:
            raise ValueError(f"at most {DSSP_MAX_RESIDUES} residues per structure, got {N}")
        if tuple(acceptor_idx.shape) != (B, N, 2) or not _is_integer_tensor(acceptor_idx):
            raise ValueError(f"acceptor_idx must be an integer tensor of shape {(B, N, 2)}, got "
                             f"{acceptor_idx.dtype} {tuple(acceptor_idx.shape)}")
    _same_device(xyz, complete=complete, junction=junction, donor=donor, acceptor_idx=acceptor_idx)


def backbone_hbonds(xyz: torch.Tensor, complete: torch.Tensor, junction: torch.Tensor,
                    donor: Optional[torch.Tensor] = None, *, n_slot: int = 0, ca_slot: int = 1, c_slot: int = 2,
                    o_slot: int = 3):
    """K21.  The backbone hydrogen bonds of DSSP, fused: ``(acceptor_idx, acceptor_energy, donor_idx, donor_energy)``, each
    (B,N,2), int32 indices and fp32 energies in kcal/mol.  ``acceptor_idx[b, j]`` are the two residues whose C=O accepts
    the N-H of residue j at the lowest Kabsch-Sander energies below -0.5 (ties to the lower index), ``donor_idx[b, i]``
    the two residues whose N-H donate to the C=O of residue i; an empty slot is index -1 and energy 0.  ``complete`` (B,N):
    the residue has N, CA, C and O and is in the residue mask; ``junction`` (B,N): r -> r+1 is a peptide bond between two
    complete residues; ``donor`` (B,N): the residue can donate (False for proline; None = all).  Pairs with CA atoms 9 A
    or more apart are not evaluated; energies are not rounded to 0.001.  Nothing of size N^2 is built; incomplete residues
    get empty lists and NaN there never reaches the result; deterministic (include/protstruc_hip.h)."""
    check_dssp_shapes(xyz, complete, junction, donor, n_slot, ca_slot, c_slot, o_slot)
    x, cm, jn, dn = _f32c(xyz, "xyz"), _u8c(complete, "complete"), _u8c(junction, "junction"), _u8c(donor, "donor")
    B, N, A = x.shape[:3]
    with _on(x.device):
        idx = [torch.full((B, N, 2), -1, dtype=torch.int32, device=x.device) for _ in range(2)]
        energy = [torch.zeros(B, N, 2, dtype=torch.float32, device=x.device) for _ in range(2)]
        if B and N:   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_backbone_hbonds_f32", _ptr(x), _ptr(cm), _ptr(jn), _ptr(dn), int(n_slot), int(ca_slot), int(c_slot),
                    int(o_slot), _ptr(idx[0]), _ptr(energy[0]), _ptr(idx[1]), _ptr(energy[1]), B, N, A, _stream(x))
    return idx[0], energy[0], idx[1], energy[1]


def dssp_assign(xyz: torch.Tensor, complete: torch.Tensor, junction: torch.Tensor, acceptor_idx: torch.Tensor, *,
                ca_slot: int = 1) -> torch.Tensor:
    """K22.  DSSP secondary-structure labels from the kept hydrogen bonds: ``codes`` (B,N) int8, indices into
    ``"-HBEGITS"``.  ``acceptor_idx`` (B,N,2) is ``backbone_hbonds``' first result; ``complete`` and ``junction`` as there;
    only the CA slot of ``xyz`` is read (the bend S).  Ladders are not joined across beta-bulges and the label is a pure
    per-residue priority H, B, E, G, I, T, S; incomplete residues get 0.  At most ``DSSP_MAX_RESIDUES`` residues per
    structure (include/protstruc_hip.h)."""
    check_dssp_shapes(xyz, complete, junction, ca_slot=ca_slot, acceptor_idx=acceptor_idx)
    x, cm, jn, acc = _f32c(xyz, "xyz"), _u8c(complete, "complete"), _u8c(junction, "junction"), _i32c(acceptor_idx, "acceptor_idx")
    B, N, A = x.shape[:3]
    with _on(x.device):
        codes = torch.zeros(B, N, dtype=torch.int8, device=x.device)
        if B and N:
            _launch("ps_dssp_assign", _ptr(x), _ptr(cm), _ptr(jn), _ptr(acc), int(ca_slot), _ptr(codes), B, N, A, _stream(x))
    return codes


SASA_MAX_SPHERE_POINTS = 256   # PS_SASA_MAX_SPHERE_POINTS of include/protstruc_hip.h: an owner's buried mask lives in registers


def check_sasa_shapes(points, radius, point_mask=None, isolate=None, sphere=None, probe=1.4) -> None:
    """Shape rules of ``solvent_accessibility``, on shapes, dtypes, devices and the scalar only (no launch): ValueError.
    ``isolate`` is an integer tensor; ``sphere`` a float32 (S,3) table with ``1 <= S <= SASA_MAX_SPHERE_POINTS`` (None is
    not checked: the layers above build it); ``probe`` non-negative and finite."""
    B, M = _points_dims(points, 2 ** 24)
    _check_float_tensor(radius, (B, M), "radius", f"points {(B, M, 3)}")
    _check_optional(point_mask, (B, M), "point_mask")
    _check_optional(isolate, (B, M), "isolate", integer=True)
    if sphere is not None:
        if not isinstance(sphere, torch.Tensor) or sphere.dtype != torch.float32 or sphere.ndim != 2 or sphere.shape[1] != 3:
            raise ValueError("sphere must be a float32 tensor of shape (S, 3), got "
                             f"{getattr(sphere, 'dtype', type(sphere).__name__)} {tuple(getattr(sphere, 'shape', ()))}")
        if not 1 <= sphere.shape[0] <= SASA_MAX_SPHERE_POINTS:
            raise ValueError(f"sphere must have between 1 and {SASA_MAX_SPHERE_POINTS} directions, got {sphere.shape[0]}")
    _check_scalar(probe, "probe", "non-negative")
    _same_device(points, radius=radius, point_mask=point_mask, isolate=isolate, sphere=sphere)


def solvent_accessibility(points: torch.Tensor, radius: torch.Tensor, point_mask: Optional[torch.Tensor] = None,
                          isolate: Optional[torch.Tensor] = None, *, sphere: torch.Tensor, probe: float = 1.4):
    """K23.  Solvent-accessible surface area by Shrake & Rupley, fused: ``(count (B,M) int32, area (B,M) fp32)``.  Point i
    carries the test points ``x_i + R_i u_k`` with ``R_i = radius_i + probe`` and ``u`` the rows of ``sphere`` (S,3;
    fp32 unit vectors, ``S <= SASA_MAX_SPHERE_POINTS``); a test point is buried where it lies inside the sphere of radius
    ``R_j`` around another point j -- both in ``point_mask`` (None = all) and, where ``isolate`` (B,M; integers) is given,
    with equal keys.  ``count_i`` is the number of test points that are not buried and ``area_i = 4 pi R_i^2 count_i / S``
    in A^2.  The decisions are taken in double on the fp32 inputs; nothing of size M^2 or M*S is built; masked points get
    zeros and NaN there (coordinates or radii) never reaches the result; deterministic (include/protstruc_hip.h)."""
    if sphere is None:
        raise ValueError("sphere is required: the (S,3) float32 table of directions (geometry.sphere_points)")
    check_sasa_shapes(points, radius, point_mask, isolate, sphere, probe)
    x, r, pm, key = _f32c(points, "points"), _f32c(radius, "radius"), _u8c(point_mask, "point_mask"), _i32c(isolate, "isolate")
    u = _f32c(sphere, "sphere")
    B, M = x.shape[:2]
    with _on(x.device):
        count = torch.zeros(B, M, dtype=torch.int32, device=x.device)
        area = torch.zeros(B, M, dtype=torch.float32, device=x.device)
        if B and M:   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_solvent_accessibility_f32", _ptr(x), _ptr(r), _ptr(pm), _ptr(key), _ptr(u), float(probe), _ptr(count),
                    _ptr(area), B, M, int(u.shape[0]), _stream(x))
    return count, area


KNN_MAX_K = 64   # PS_KNN_MAX_K of include/protstruc_hip.h: an owner's list of k lives in LDS


def _check_neighbor_operands(points, B, M, point_mask, queries, query_mask, exclude, query_exclude, include_self) -> int:
    """The masks, keys and queries of a neighbour list over ``points`` (B,M,3), as ``check_knn_shapes`` states them:
    ValueError; returns Q, the queries per structure (M in the self graph)."""
    _check_optional(point_mask, (B, M), "point_mask", "points", (B, M, 3))
    _check_optional(exclude, (B, M), "exclude", "points", (B, M, 3), integer=True)
    Q = M
    if queries is None:
        for name, t in (("query_mask", query_mask), ("query_exclude", query_exclude)):
            if t is not None:
                raise ValueError(f"{name} needs queries: in the self graph the points' own mask and keys are used")
    else:
        shape = tuple(queries.shape)
        if len(shape) != 3 or shape[2] != 3 or shape[0] != B:
            raise ValueError(f"queries must have shape ({B}, queries, 3) to match points {(B, M, 3)}, got {shape}")
        if not queries.dtype.is_floating_point:
            raise ValueError(f"queries must be a floating-point tensor, got {queries.dtype}")
        Q = shape[1]
        _check_count(Q, 0, 2 ** 24, "queries per structure")
        _check_optional(query_mask, (B, Q), "query_mask", "queries", shape)
        _check_optional(query_exclude, (B, Q), "query_exclude", "queries", shape, integer=True)
        if (exclude is None) != (query_exclude is None):
            raise ValueError("exclude and query_exclude come together: a candidate is skipped where the two keys are equal")
        if include_self:
            raise ValueError("include_self applies to the self graph only (queries=None)")
    _same_device(points, point_mask=point_mask, queries=queries, query_mask=query_mask, exclude=exclude,
                 query_exclude=query_exclude)
    return Q


def check_knn_shapes(points, k, point_mask=None, queries=None, query_mask=None, exclude=None, query_exclude=None,
                     cutoff=_INF, include_self=False) -> None:
    """Shape rules of ``nearest_neighbors``, on shapes, dtypes, devices and the scalars only (no launch): ValueError.
    ``1 <= k <= KNN_MAX_K``; ``cutoff`` positive, +inf allowed; ``exclude`` / ``query_exclude`` integer tensors.  Without
    ``queries`` (the self graph) ``query_mask`` and ``query_exclude`` are not given -- they are ``point_mask`` and
    ``exclude``; with ``queries``, ``exclude`` and ``query_exclude`` come together and ``include_self`` means nothing."""
    B, M = _points_dims(points, 2 ** 24)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k must be an integer in 1 .. {KNN_MAX_K}, got {k!r}")
    if float(cutoff) != _INF:
        _check_scalar(cutoff, "cutoff", "positive")
    _check_neighbor_operands(points, B, M, point_mask, queries, query_mask, exclude, query_exclude, include_self)


def nearest_neighbors(points: torch.Tensor, k: int, point_mask: Optional[torch.Tensor] = None, *,
                      queries: Optional[torch.Tensor] = None, query_mask: Optional[torch.Tensor] = None,
                      exclude: Optional[torch.Tensor] = None, query_exclude: Optional[torch.Tensor] = None,
                      cutoff: float = _INF, include_self: bool = False):
    """K24.  The k nearest neighbours of every query, fused and sorted: ``(idx (B,Q,k) int32, dist (B,Q,k) fp32, count
    (B,Q) int32)``.  ``points`` (B,M,3) are the candidates, ``queries`` (B,Q,3) the points asked for -- None: the points
    themselves (the self graph, Q = M, where a point is not its own neighbour unless ``include_self``).  A candidate j is a
    neighbour of query q where both are in their masks (``point_mask`` (B,M), ``query_mask`` (B,Q); None = all; the self
    graph uses ``point_mask`` for both), their keys differ (``exclude`` (B,M), ``query_exclude`` (B,Q), integers: the
    residue index for atom graphs, the chain index for interface graphs), the squared distance ``d2 = (dx*dx + dy*dy) +
    dz*dz``, evaluated in double on the float32 inputs, is finite and ``d2 <= cutoff^2``.  The neighbours are ordered by
    ``(d2, j)`` -- equal distances to the lower index -- and the first ``k <= KNN_MAX_K`` kept: ``idx`` indexes the M axis
    (padding -1), ``dist = sqrt(d2)`` rounded to float32 once (padding +inf), ``count`` is the number of real neighbours.
    A masked query gets count 0 and all padding; a NaN or infinite coordinate makes a point nobody's neighbour, and NaN
    under a mask never reaches arithmetic.  Nothing of size Q*M is built; deterministic (include/protstruc_hip.h)."""
    check_knn_shapes(points, k, point_mask, queries, query_mask, exclude, query_exclude, cutoff, include_self)
    x, pm, key = _f32c(points, "points"), _u8c(point_mask, "point_mask"), _i32c(exclude, "exclude")
    y, qm, qkey = _f32c_opt(queries, "queries"), _u8c(query_mask, "query_mask"), _i32c(query_exclude, "query_exclude")
    B, M = x.shape[:2]
    Q, k = M if y is None else y.shape[1], int(k)
    with _on(x.device):
        if not (B and M and Q):   # empty input: nothing to launch (an empty tensor has no device pointer)
            return (torch.full((B, Q, k), -1, dtype=torch.int32, device=x.device),
                    torch.full((B, Q, k), _INF, dtype=torch.float32, device=x.device),
                    torch.zeros(B, Q, dtype=torch.int32, device=x.device))
        idx = torch.empty(B, Q, k, dtype=torch.int32, device=x.device)   # the kernel writes every element
        dist = torch.empty(B, Q, k, dtype=torch.float32, device=x.device)
        count = torch.empty(B, Q, dtype=torch.int32, device=x.device)
        _launch("ps_nearest_neighbors_f32", _ptr(x), _ptr(pm), _ptr(y), _ptr(qm), _ptr(key), _ptr(qkey), k, float(cutoff),
                int(bool(include_self)), _ptr(idx), _ptr(dist), _ptr(count), B, M, Q, _stream(x))
    return idx, dist, count


RADIUS_TILE = 64  # PS_RADIUS_TILE of include/protstruc_graph.h
RADIUS_BOX_FLOATS = 40   # PS_RADIUS_BOX_FLOATS: five boxes of eight floats per block of candidates
RADIUS_STATS = 6   # PS_RADIUS_STATS: counters per wave of 64 queries


def check_radius_graph_shapes(points, cutoff, point_mask=None, queries=None, query_mask=None, exclude=None,
                              query_exclude=None, include_self=False, max_edges=None) -> Tuple[int, int, int]:
    """Shape rules of ``radius_graph``, on shapes, dtypes, devices and the scalars only (no launch): ValueError; returns
    (B, M, Q).  K24's rules (``check_knn_shapes``) without a ``k``, except that ``cutoff`` is positive AND finite, and
    ``max_edges`` is None or a non-negative integer."""
    B, M = _points_dims(points, 2 ** 24)
    _check_scalar(cutoff, "cutoff", "positive")
    if max_edges is not None:
        if isinstance(max_edges, bool) or not isinstance(max_edges, (int, np.integer)) or max_edges < 0:
            raise ValueError(f"max_edges must be None or a non-negative integer, got {max_edges!r}")
    Q = _check_neighbor_operands(points, B, M, point_mask, queries, query_mask, exclude, query_exclude, include_self)
    return B, M, Q


def radius_graph(points: torch.Tensor, cutoff: float, point_mask: Optional[torch.Tensor] = None, *,
                 queries: Optional[torch.Tensor] = None, query_mask: Optional[torch.Tensor] = None,
                 exclude: Optional[torch.Tensor] = None, query_exclude: Optional[torch.Tensor] = None,
                 include_self: bool = False, max_edges: Optional[int] = None, return_stats: bool = False):
    """K47 + K48.  Every neighbour of every query within ``cutoff``, as lists of any length in CSR form: ``(row_ptr
    (B*Q+1,) int64, col (E,) int32, dist (E,) fp32, count (B,Q) int32)``.  The arguments and the predicate are those of
    ``nearest_neighbors`` -- masks, keys, the self graph without ``queries``, ``d2`` in double on the float32 inputs,
    ``d2 <= cutoff^2`` inclusive -- with no ``k`` and no cap: row ``b * Q + q`` is ``col[row_ptr[r]:row_ptr[r + 1]]``, the
    neighbours' indices into the M axis of structure b, ASCENDING, and ``dist = sqrt(d2)`` rounded to float32 once.
    A masked query or one with a non-finite coordinate has an empty row.

    ``max_edges=None`` reads ``row_ptr[-1]`` from the device once, to size ``col`` and ``dist``: a host read, so not
    capturable.  ``max_edges=n`` makes none: ``col`` and ``dist`` have n entries, an edge whose position is >= n is not
    written, ``row_ptr`` and ``count`` stay exact (test ``row_ptr[-1] <= n``), and the entries past ``row_ptr[-1]`` are
    -1 / +inf; this form runs inside a captured graph.  Three launches (boxes, count, fill) and a ``torch.cumsum``;
    nothing of size Q*M is built; no atomics, deterministic (include/protstruc_graph.h).  ``return_stats`` appends the
    counting sweep's (B, ceil(Q/64), RADIUS_STATS) int32 counters."""
    B, M, Q = check_radius_graph_shapes(points, cutoff, point_mask, queries, query_mask, exclude, query_exclude, include_self,
                                        max_edges)
    x, pm, key = _f32c(points, "points"), _u8c(point_mask, "point_mask"), _i32c(exclude, "exclude")
    y, qm, qkey = _f32c_opt(queries, "queries"), _u8c(query_mask, "query_mask"), _i32c(query_exclude, "query_exclude")
    rows, waves = B * Q, (Q + 63) // 64
    with _on(x.device):
        row_ptr = torch.zeros(rows + 1, dtype=torch.int64, device=x.device)
        stats = torch.zeros(B, waves, RADIUS_STATS, dtype=torch.int32, device=x.device) if return_stats else None
        if not (B and M and Q):   # empty input: nothing to launch (an empty tensor has no device pointer)
            n = 0 if max_edges is None else int(max_edges)
            out = (row_ptr, torch.full((n,), -1, dtype=torch.int32, device=x.device),
                   torch.full((n,), _INF, dtype=torch.float32, device=x.device),
                   torch.zeros(B, Q, dtype=torch.int32, device=x.device))
            return out + (stats,) if return_stats else out
        boxes = torch.empty(B, (M + RADIUS_TILE - 1) // RADIUS_TILE, RADIUS_BOX_FLOATS, dtype=torch.float32, device=x.device)
        count = torch.empty(B, Q, dtype=torch.int32, device=x.device)   # the kernel writes every element
        stream = _stream(x)
        inputs = (_ptr(x), _ptr(pm), _ptr(y), _ptr(qm), _ptr(key), _ptr(qkey), float(cutoff), int(bool(include_self)), _ptr(boxes))
        _launch("ps_radius_tile_boxes_f32", _ptr(x), _ptr(pm), _ptr(boxes), B, M, stream)
        _launch("ps_radius_count_f32", *inputs, _ptr(count), _ptr(stats), B, M, Q, stream)
        torch.cumsum(count.reshape(-1), 0, dtype=torch.int64, out=row_ptr[1:])
        if max_edges is None:
            n = int(row_ptr[-1].item())   # the documented host read
            col = torch.empty(n, dtype=torch.int32, device=x.device)   # the kernel writes every element
            dist = torch.empty(n, dtype=torch.float32, device=x.device)
        else:
            n = int(max_edges)
            col = torch.full((n,), -1, dtype=torch.int32, device=x.device)
            dist = torch.full((n,), _INF, dtype=torch.float32, device=x.device)
        if n:
            _launch("ps_radius_fill_f32", *inputs, _ptr(row_ptr), n, _ptr(col), _ptr(dist), B, M, Q, stream)
    out = (row_ptr, col, dist, count)
    return out + (stats,) if return_stats else out


CLOSEST_MAX_ATOMS = 64         # PS_CLOSEST_MAX_ATOMS of include/protstruc_contacts.h: a residue's presence word is 64 bits
CLOSEST_MAX_RESIDUES = 2 ** 20  # PS_CLOSEST_MAX_RESIDUES


def check_closest_atoms_shapes(xyz, atom_mask=None, cutoff=_INF, pair=None, grad_dist=None) -> None:
    """Shape rules of ``closest_atoms`` / ``closest_atoms_backward``, on shapes, dtypes, devices and the scalar only (no
    launch): ValueError.  ``xyz`` (B,N,A,3) floating point with ``B <= MAX_BATCH``, ``1 <= N <= CLOSEST_MAX_RESIDUES`` and ``1 <=
    A <= CLOSEST_MAX_ATOMS``; ``atom_mask`` (B,N,A); ``cutoff`` non-negative, +inf allowed; for the backward pass ``pair``
    (B,N,N) integers and ``grad_dist`` (B,N,N) floating point."""
    B, N, A = _xyz_dims(xyz)
    shape = (B, N, A, 3)
    _check_batch(B)
    _check_count(N, 1, CLOSEST_MAX_RESIDUES, "residues per structure")
    _check_count(A, 1, CLOSEST_MAX_ATOMS, "atom slots per residue")
    _check_optional(atom_mask, (B, N, A), "atom_mask", "xyz", shape)
    if float(cutoff) != _INF:
        _check_scalar(cutoff, "cutoff", "non-negative")
    _check_optional(pair, (B, N, N), "pair", "xyz", shape, integer=True)
    _check_optional(grad_dist, (B, N, N), "grad_dist", "xyz", shape, floating=True)
    _same_device(xyz, atom_mask=atom_mask, pair=pair, grad_dist=grad_dist)


def closest_atoms(xyz: torch.Tensor, atom_mask: Optional[torch.Tensor] = None, cutoff: float = _INF):
    """K31.  The closest atoms of every pair of residues, fused: ``(dist (B,N,N) fp32, pair (B,N,N) int16)``.  Over every
    atom a of residue i and atom c of residue j that are in ``atom_mask`` (B,N,A; None = all), ``d2 = (dx*dx + dy*dy) +
    dz*dz`` in double on the float32 coordinates; non-finite ``d2`` are skipped, the minimum under ``(d2, a, c)`` -- ties
    to the lower a, then the lower c, for i <= j -- counts where ``d2 <= cutoff^2``: ``dist = sqrt(d2)`` rounded to float32
    once and ``pair = a * A + c``; ``dist = +inf`` and ``pair = -1`` where nothing counts.  Entry (j,i) mirrors (i,j): the
    same ``dist`` bits and ``pair = c * A + a``, so ``pair[b,r,s]`` reads (atom of r, atom of s).  The diagonal is not
    special (0.0 and the lowest present slot twice).  NaN under the mask never reaches a result; a finite ``cutoff`` lets
    the kernel skip residue pairs that are far apart without changing a bit.  Nothing of size N*N*A*A is built;
    deterministic (include/protstruc_contacts.h)."""
    check_closest_atoms_shapes(xyz, atom_mask, cutoff)
    x, am = _f32c(xyz, "xyz"), _u8c(atom_mask, "atom_mask")
    B, N, A = x.shape[:3]
    with _on(x.device):
        dist = torch.empty(B, N, N, dtype=torch.float32, device=x.device)   # the kernel writes every element
        pair = torch.empty(B, N, N, dtype=torch.int16, device=x.device)
        if B:   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_closest_atoms_f32", _ptr(x), _ptr(am), _ptr(dist), _ptr(pair), B, N, A, float(cutoff), _stream(x))
    return dist, pair


def closest_atoms_backward(xyz: torch.Tensor, pair: torch.Tensor, grad_dist: torch.Tensor) -> torch.Tensor:
    """K32.  Vector-Jacobian product of ``closest_atoms`` towards the coordinates in one launch: ``grad_xyz`` (B,N,A,3)
    fp32 from ``pair`` (B,N,N), as the forward pass returned it, and the upstream ``grad_dist`` (B,N,N).  Slot a of residue
    i collects ``(g[i,j] + g[j,i]) (Xia - Xjc) / |Xia - Xjc|`` over the j != i whose recorded pair is (a, c), over j
    ascending in double, rounded once; a pair of -1 (any value outside [0, A*A)) and a distance of 0 contribute nothing,
    so the gradient at ``dist = +inf`` is dropped; exact zeros in the slots that win no pair.  No atomics, deterministic
    (include/protstruc_contacts.h)."""
    check_closest_atoms_shapes(xyz, None, _INF, pair, grad_dist)
    x, g = _f32c(xyz, "xyz"), _f32c(grad_dist, "grad_dist")
    B, N, A = x.shape[:3]
    _require_device(pair, "pair")
    if pair.dtype != torch.int16:   # wider integers: everything out of range becomes -1 first, so that none wraps into it
        pair = torch.where((pair >= 0) & (pair < A * A), pair, torch.full_like(pair, -1)).to(torch.int16)
    p = pair.contiguous()
    with _on(x.device):
        out = torch.empty(B, N, A, 3, dtype=torch.float32, device=x.device)
        if B:
            _launch("ps_closest_atoms_backward_f32", _ptr(x), _ptr(p), _ptr(g), _ptr(out), B, N, A, _stream(x))
    return out


PAIRHEAD_MAX_RESIDUES = 2 ** 20  # PS_PAIRHEAD_MAX_RESIDUES of include/protstruc_pairhead.h
PAIRHEAD_MAX_BREAKS = 127        # PS_PAIRHEAD_MAX_BREAKS: every bin index and the "no target" label fit a byte
PAIRHEAD_MAX_BINS = 128          # PS_PAIRHEAD_MAX_BINS
PAIRHEAD_MAX_TABLES = 4          # PS_PAIRHEAD_MAX_TABLES
PAIRHEAD_NO_TARGET = 255         # PS_PAIRHEAD_NO_TARGET: the bin of a pair without a target


def _check_breaks(breaks) -> np.ndarray:
    """``breaks`` as the float32 host array the launcher reads: 1 .. PAIRHEAD_MAX_BREAKS finite, non-negative, strictly
    increasing numbers; ValueError otherwise."""
    arr = np.ascontiguousarray(_host_f32(breaks, "breaks"))
    _check_count(arr.size, 1, PAIRHEAD_MAX_BREAKS, "breaks")
    if not (np.isfinite(arr).all() and (arr >= 0).all() and (np.diff(arr) > 0).all()):
        raise ValueError("breaks must be finite, non-negative and strictly increasing")
    return arr


def _pair_batch(B: int, N: int) -> None:
    _check_batch(B)
    _check_count(N, 1, PAIRHEAD_MAX_RESIDUES, "residues per structure")


def check_pair_bins_shapes(points, breaks, row_mask=None, col_mask=None, rot=None, trans=None, target_rot=None,
                           target_trans=None, target_points=None) -> None:
    """Shape rules of ``pair_bins_distance`` / ``pair_bins_aligned_error``, on shapes, dtypes, devices and the host table
    only (no launch): ValueError.  ``points`` (B,N,3) floating point with ``B <= MAX_BATCH`` and ``1 <= N <=
    PAIRHEAD_MAX_RESIDUES``; the masks (B,N); ``breaks`` 1 .. ``PAIRHEAD_MAX_BREAKS`` finite, non-negative, strictly
    increasing numbers; with ``rot`` given (the aligned error) ``rot`` and ``target_rot`` (B,N,3,3), ``trans``,
    ``target_trans`` and ``target_points`` (B,N,3), all floating point."""
    shape = _float_dims(points, "points", "batch, residues, 3")
    B, N = shape[:2]
    _pair_batch(B, N)
    _check_breaks(breaks)
    _check_optional(row_mask, (B, N), "row_mask", "points", shape)
    _check_optional(col_mask, (B, N), "col_mask", "points", shape)
    frames = {} if rot is None else dict(rot=rot, trans=trans, target_rot=target_rot, target_trans=target_trans,
                                         target_points=target_points)
    for name, t in frames.items():
        _check_float_tensor(t, (B, N, 3, 3) if name.endswith("rot") else (B, N, 3), name, f"points {shape}")
    _same_device(points, row_mask=row_mask, col_mask=col_mask, **frames)


def _pair_bins(mode, floats, row_mask, col_mask, breaks, return_value):
    points = floats[0]
    B, N = points.shape[:2]
    rm, cm = _u8c(row_mask, "row_mask"), _u8c(col_mask, "col_mask")
    table = _check_breaks(breaks)
    with _on(points.device):
        bins = torch.empty(B, N, N, dtype=torch.uint8, device=points.device)    # the kernel writes every element
        value = torch.empty(B, N, N, dtype=torch.float32, device=points.device) if return_value else None
        if B:   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_pair_bins_f32", mode, *[_ptr(t) for t in floats], _ptr(rm), _ptr(cm), table.ctypes.data, int(table.size),
                    _ptr(bins), _ptr(value), B, N, _stream(points))
    return (bins, value) if return_value else bins


def pair_bins_distance(points: torch.Tensor, breaks, row_mask: Optional[torch.Tensor] = None,
                       col_mask: Optional[torch.Tensor] = None, return_value: bool = False):
    """K33, distance mode.  The distogram bin of every pair of ``points`` (B,N,3): ``bins`` (B,N,N) uint8 with ``bins[b,i,j] =
    #{k : d2 > breaks[k]^2}`` -- AlphaFold's ``sum(d2 > sq_breaks)`` --, where ``d2 = (dx*dx + dy*dy) + dz*dz`` with ``dx = xj -
    xi`` and the squared breaks are formed in double on the float32 inputs, so the bin is defined bit for bit.  ``breaks`` is
    a host sequence of 1 .. 127 finite, non-negative, strictly increasing numbers.  Where ``row_mask[b,i] * col_mask[b,j]``
    (B,N; None = all) is 0 or ``d2`` is not finite the bin is ``PAIRHEAD_NO_TARGET`` (255); NaN under a mask never reaches
    an output.  With ``return_value`` also ``value`` (B,N,N) fp32, ``sqrt(d2)`` rounded to float32 once, +inf where the
    bin is 255 (include/protstruc_pairhead.h)."""
    check_pair_bins_shapes(points, breaks, row_mask, col_mask)
    return _pair_bins(0, [_f32c(points, "points")] + [None] * 5, row_mask, col_mask, breaks, return_value)


def pair_bins_aligned_error(rot: torch.Tensor, trans: torch.Tensor, points: torch.Tensor, target_rot: torch.Tensor,
                            target_trans: torch.Tensor, target_points: torch.Tensor, breaks,
                            frame_mask: Optional[torch.Tensor] = None, point_mask: Optional[torch.Tensor] = None,
                            return_value: bool = False):
    """K33, aligned-error mode.  The bin of the aligned error ``|R_i^T (x_j - t_i) - R*_i^T (x*_j - t*_i)|`` of every (frame i,
    point j): ``bins`` (B,N,N) uint8, counted over ``breaks`` as in ``pair_bins_distance``, the error's square formed in
    double on the float32 inputs in a stated order.  ``rot`` (B,N,3,3) has the basis vectors as columns, as ``frames``
    returns it; ``points`` (B,N,3) is one point per residue.  The row mask is ``frame_mask``, the column mask
    ``point_mask`` (B,N; None = all); 255 where either is 0 or the error is not finite.  With ``return_value`` also the
    error itself, (B,N,N) fp32, +inf where the bin is 255 (include/protstruc_pairhead.h)."""
    check_pair_bins_shapes(points, breaks, frame_mask, point_mask, rot, trans, target_rot, target_trans, target_points)
    floats = [_f32c(t, name) for t, name in ((points, "points"), (rot, "rot"), (trans, "trans"), (target_points, "target_points"),
                                             (target_rot, "target_rot"), (target_trans, "target_trans"))]
    return _pair_bins(1, floats, frame_mask, point_mask, breaks, return_value)


def check_binned_shapes(logits, bins=None, grad_row=None, values=None) -> None:
    """Shape rules of ``binned_cross_entropy``, ``binned_cross_entropy_backward`` and ``binned_expectation``, on shapes,
    dtypes and devices only (no launch): ValueError.  ``logits`` (B,N,N,C) floating point with ``B <= MAX_BATCH``, ``1 <= N <=
    PAIRHEAD_MAX_RESIDUES`` and ``2 <= C <= PAIRHEAD_MAX_BINS``; ``bins`` (B,N,N) integers; ``grad_row`` (B,N) floating
    point; ``values`` (B,V,C) floating point with ``1 <= V <= PAIRHEAD_MAX_TABLES``."""
    shape = tuple(logits.shape)
    if len(shape) != 4 or shape[1] != shape[2]:
        raise ValueError(f"logits must have shape (batch, residues, residues, bins), got {shape}")
    if not logits.dtype.is_floating_point:
        raise ValueError(f"logits must be a floating-point tensor, got {logits.dtype}")
    B, N, _, C = shape
    _pair_batch(B, N)
    _check_count(C, 2, PAIRHEAD_MAX_BINS, "bins")
    _check_optional(bins, (B, N, N), "bins", "logits", shape, integer=True)
    _check_optional(grad_row, (B, N), "grad_row", "logits", shape, floating=True)
    if values is not None:
        vshape = tuple(values.shape)
        if len(vshape) != 3 or vshape[0] != B or vshape[2] != C:
            raise ValueError(f"values must have shape ({B}, tables, {C}) to match logits {shape}, got {vshape}")
        _check_count(vshape[1], 1, PAIRHEAD_MAX_TABLES, "value tables")
        if not values.dtype.is_floating_point:
            raise ValueError(f"values must be a floating-point tensor, got {values.dtype}")
    _same_device(logits, bins=bins, grad_row=grad_row, values=values)


def _bins_u8(bins: torch.Tensor, C: int) -> torch.Tensor:
    _require_device(bins, "bins")
    if bins.dtype != torch.uint8:   # wider integers: everything outside [0, C) becomes 255 first, so that nothing wraps into range
        bins = torch.where((bins >= 0) & (bins < C), bins, torch.full_like(bins, PAIRHEAD_NO_TARGET)).to(torch.uint8)
    return bins.contiguous()


def binned_cross_entropy(logits: torch.Tensor, bins: torch.Tensor):
    """K34.  Cross-entropy of ``logits`` (B,N,N,C) against the labels ``bins`` (B,N,N), summed per row in one pass over the
    logits: ``(row_loss (B,N) fp32, row_count (B,N) int32)`` with ``row_loss[b,i] = sum_j lse(x_ij) - x_ij[bins_ij]`` over
    the ``j`` whose label is in ``[0, C)`` and ``row_count`` their number.  A label outside ``[0, C)`` -- the 255 of "no
    target" -- contributes nothing and the logits there, NaN included, never reach the sum; ``-inf`` logits are legal.
    Labels that are not uint8 are mapped to uint8 first, everything outside ``[0, C)`` to 255.  Per pair fp32; across
    ``j`` double in a fixed order, rounded once: no atomics, deterministic.  No log-softmax tensor is built
    (include/protstruc_pairhead.h)."""
    check_binned_shapes(logits, bins)
    x = _f32c(logits, "logits")
    B, N, _, C = x.shape
    b = _bins_u8(bins, C)
    with _on(x.device):
        row_loss = torch.empty(B, N, dtype=torch.float32, device=x.device)   # the kernel writes every element
        row_count = torch.empty(B, N, dtype=torch.int32, device=x.device)
        if B:
            _launch("ps_binned_cross_entropy_f32", _ptr(x), _ptr(b), _ptr(row_loss), _ptr(row_count), B, N, C, _stream(x))
    return row_loss, row_count


def binned_cross_entropy_backward(logits: torch.Tensor, bins: torch.Tensor, grad_row: torch.Tensor) -> torch.Tensor:
    """K35.  Vector-Jacobian product of ``binned_cross_entropy`` towards the logits: ``grad_logits`` (B,N,N,C) fp32 with
    ``grad_row[b,i] * (softmax(x_ij)_k - [k == bins_ij])`` and exact zeros, all C of them, where the label is outside
    ``[0, C)``.  One pass: reads the logits once and writes every element once (include/protstruc_pairhead.h)."""
    check_binned_shapes(logits, bins, grad_row)
    x, g = _f32c(logits, "logits"), _f32c(grad_row, "grad_row")
    B, N, _, C = x.shape
    b = _bins_u8(bins, C)
    with _on(x.device):
        out = torch.empty(B, N, N, C, dtype=torch.float32, device=x.device)
        if B:
            _launch("ps_binned_cross_entropy_backward_f32", _ptr(x), _ptr(b), _ptr(g), _ptr(out), B, N, C, _stream(x))
    return out


def binned_expectation(logits: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
    """K36.  Expectations under the softmax of ``logits`` (B,N,N,C): ``out`` (V,B,N,N) fp32 with ``out[v,b,i,j] = sum_k
    softmax(x_ij)_k * values[b,v,k]`` for the ``1 <= V <= 4`` tables ``values`` (B,V,C).  One pass over the logits serves all
    tables; no softmax tensor is built (include/protstruc_pairhead.h)."""
    check_binned_shapes(logits, values=values)
    x, v = _f32c(logits, "logits"), _f32c(values, "values")
    B, N, _, C = x.shape
    V = v.shape[1]
    with _on(x.device):
        out = torch.empty(V, B, N, N, dtype=torch.float32, device=x.device)
        if B:
            _launch("ps_binned_expectation_f32", _ptr(x), _ptr(v), _ptr(out), B, N, C, V, _stream(x))
    return out


SUPERPOSE_MAX_POINTS = 2048     # PS_SUPERPOSE_MAX_POINTS of include/protstruc_superpose.h: the search keeps a structure's pairs in LDS
SUPERPOSE_MAX_OBJECTIVES = 8    # PS_SUPERPOSE_MAX_OBJECTIVES
SUPERPOSE_TM = 0                # PS_SUPERPOSE_TM: the objective 1 / (1 + d^2 / d0^2), param d0
SUPERPOSE_COUNT = 1             # PS_SUPERPOSE_COUNT: the objective [d <= c], param c


def check_superpose_shapes(a, b, weight=None, mask=None, grad_rmsd=None, l_norm=None, max_points=None) -> Tuple[int, int, bool]:
    """Shape rules of ``superpose``, ``superpose_backward`` and ``superpose_search``, on shapes, dtypes and devices only (no
    launch): ValueError.  ``a`` (B,M,3) floating point with ``B <= MAX_BATCH`` and ``M >= 1`` (``M <= max_points`` where given);
    ``b`` (B,M,3), or (1,M,3) as one target for all; ``weight`` (B,M) floating point; ``mask`` (B,M); ``grad_rmsd`` and
    ``l_norm`` (B,) floating point.  Returns (B, M, one target for all)."""
    shape = _float_dims(a, "a", "batch, points, 3")
    B, M = shape[:2]
    _check_batch(B)
    _check_count(M, 1, max_points, "points per structure")
    if tuple(b.shape) != shape and tuple(b.shape) != (1, M, 3):
        raise ValueError(f"b must have shape {shape} or {(1, M, 3)} to match a, got {tuple(b.shape)}")
    if not b.dtype.is_floating_point:
        raise ValueError(f"b must be a floating-point tensor, got {b.dtype}")
    _check_optional(weight, (B, M), "weight", "a", shape, floating=True)
    _check_optional(mask, (B, M), "mask", "a", shape)
    _check_optional(grad_rmsd, (B,), "grad_rmsd", "a", shape, floating=True)
    _check_optional(l_norm, (B,), "l_norm", "a", shape, floating=True)
    _same_device(a, b=b, weight=weight, mask=mask, grad_rmsd=grad_rmsd, l_norm=l_norm)
    return B, M, tuple(b.shape) != shape


def superpose(a: torch.Tensor, b: torch.Tensor, weight: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None):
    """K37.  The weighted optimal superposition of ``a`` (B,M,3) onto ``b`` (B,M,3), or (1,M,3) as one target for all, with
    its RMSD: ``(R (B,3,3), t (B,3), rmsd (B,), wsum (B,))`` fp32.  Over the points with ``mask`` (B,M; None = all) set and
    ``weight`` (B,M; None = 1) above 0: weighted centroids, the covariance about them, the 3x3 solve of ``kabsch`` -- always
    a proper rotation --, and ``rmsd = sqrt(sum w |R a + t - b|^2 / sum w)`` from a pass of its own over the residuals, all in
    double on the float32 inputs, so identical inputs give an RMSD at the rounding of the coordinates.  ``wsum = sum w``;
    where it is 0, ``R``, ``t`` and ``rmsd`` are NaN.  Entries under the mask and coordinates at weight 0 are never read
    (include/protstruc_superpose.h)."""
    B, M, shared = check_superpose_shapes(a, b, weight, mask)
    x, y, w, m = _f32c(a, "a"), _f32c(b, "b"), _f32c_opt(weight, "weight"), _u8c(mask, "mask")
    dev = x.device
    with _on(dev):
        R = torch.empty(B, 3, 3, dtype=torch.float32, device=dev)       # the kernel writes every element
        t = torch.empty(B, 3, dtype=torch.float32, device=dev)
        rmsd = torch.empty(B, dtype=torch.float32, device=dev)
        wsum = torch.empty(B, dtype=torch.float32, device=dev)
        if B:   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_superpose_f32", _ptr(x), _ptr(y), _ptr(w), _ptr(m), _ptr(R), _ptr(t), _ptr(rmsd), _ptr(wsum), B, M,
                    int(shared), _stream(x))
    return R, t, rmsd, wsum


def superpose_backward(a: torch.Tensor, b: torch.Tensor, weight: Optional[torch.Tensor], mask: Optional[torch.Tensor],
                       R: torch.Tensor, t: torch.Tensor, rmsd: torch.Tensor, wsum: torch.Tensor, grad_rmsd: torch.Tensor):
    """K38.  Vector-Jacobian product of ``superpose``'s ``rmsd`` towards the points: ``(grad_a (B,M,3), grad_b (B,M,3))``
    fp32, ``grad_b`` None where ``b`` is one target for all (a constant).  At the optimum the derivative through ``R`` and
    ``t`` vanishes: ``grad_a_i = g w_i R^T e_i / (wsum rmsd)`` and ``grad_b_i = -g w_i e_i / (wsum rmsd)`` with ``e_i = R a_i +
    t - b_i``.  ``R``, ``t`` and the weights get no gradient.  Exact zeros under the mask, at weight 0, and for a
    structure whose ``rmsd`` is 0 or not finite or whose ``R`` holds NaN; every element is written once.  ``R``, ``t``, ``rmsd``
    and ``wsum`` are what ``superpose`` returned for the same inputs (include/protstruc_superpose.h)."""
    B, M, shared = check_superpose_shapes(a, b, weight, mask, grad_rmsd)
    x, y, w, m = _f32c(a, "a"), _f32c(b, "b"), _f32c_opt(weight, "weight"), _u8c(mask, "mask")
    dev = x.device
    for name, value, want in (("R", R, (B, 3, 3)), ("t", t, (B, 3)), ("rmsd", rmsd, (B,)), ("wsum", wsum, (B,))):
        _check_out(value, want, name, dev)
    g = _f32c(grad_rmsd, "grad_rmsd")
    with _on(dev):
        grad_a = torch.empty(B, M, 3, dtype=torch.float32, device=dev)
        grad_b = None if shared else torch.empty(B, M, 3, dtype=torch.float32, device=dev)
        if B:
            _launch("ps_superpose_backward_f32", _ptr(x), _ptr(y), _ptr(w), _ptr(m), _ptr(R), _ptr(t), _ptr(rmsd), _ptr(wsum),
                    _ptr(g), _ptr(grad_a), _ptr(grad_b), B, M, int(shared), _stream(x))
    return grad_a, grad_b


def _check_objectives(objectives):
    """``objectives`` -- 1 .. SUPERPOSE_MAX_OBJECTIVES pairs (kind, param) -- as the host array the launcher reads"""
    pairs = [(int(kind), float(param)) for kind, param in objectives]
    _check_count(len(pairs), 1, SUPERPOSE_MAX_OBJECTIVES, "objectives")
    for kind, param in pairs:
        if kind not in (SUPERPOSE_TM, SUPERPOSE_COUNT):
            raise ValueError(f"an objective's kind is SUPERPOSE_TM (0) or SUPERPOSE_COUNT (1), got {kind}")
        _check_scalar(param, "an objective's param", "positive")
    return (_lib.SuperposeObjective * len(pairs))(*[_lib.SuperposeObjective(kind, param) for kind, param in pairs])


def superpose_search(a: torch.Tensor, b: torch.Tensor, mask: Optional[torch.Tensor], l_norm: torch.Tensor, objectives):
    """K39 / K40.  The seeded search for the superposition of ``a`` (B,M,3) onto ``b`` (B,M,3) that maximises each of up to
    eight ``objectives`` -- a host sequence of ``(kind, param)``: ``(SUPERPOSE_TM, d0)`` sums ``1 / (1 + d^2 / d0^2)`` over the
    points, ``(SUPERPOSE_COUNT, c)`` counts the points with ``d <= c`` --: ``(score (B,n_obj), R (B,n_obj,3,3), t (B,n_obj,3))``
    fp32, ``score`` the best sum divided by ``l_norm`` (B,), with the transform that attains it.  ``M <=
    SUPERPOSE_MAX_POINTS``; the points are those with ``mask`` (B,M; None = all) set, and entries under the mask are never
    read.  The procedure -- fragment seeds, iterated selection within a radius, at most 20 fits per chain -- is defined in
    include/protstruc_superpose.h and is deterministic: no atomics, repeated runs agree bit for bit.  A structure without
    points scores 0 with NaN transforms.  Not differentiable."""
    B, M, shared = check_superpose_shapes(a, b, None, mask, None, l_norm, SUPERPOSE_MAX_POINTS)
    table = _check_objectives(objectives)
    n_obj = len(table)
    x, y, m, ln = _f32c(a, "a"), _f32c(b, "b"), _u8c(mask, "mask"), _f32c(l_norm, "l_norm")
    if shared:
        y = y.expand(B, M, 3).contiguous()
    dev = x.device
    with _on(dev):
        score = torch.empty(B, n_obj, dtype=torch.float32, device=dev)       # the kernels write every element
        R = torch.empty(B, n_obj, 3, 3, dtype=torch.float32, device=dev)
        t = torch.empty(B, n_obj, 3, dtype=torch.float32, device=dev)
        if B:
            floats = _lib.load().ps_superpose_workspace_floats(B, M, n_obj)
            workspace = torch.empty(floats, dtype=torch.float32, device=dev)
            _launch("ps_superpose_search_f32", _ptr(x), _ptr(y), _ptr(m), _ptr(ln), ctypes.addressof(table), n_obj,
                    _ptr(workspace), _ptr(score), _ptr(R), _ptr(t), B, M, _stream(x))
    return score, R, t


STRUCTALIGN_MAX_POINTS = 1024   # PS_STRUCTALIGN_MAX_POINTS of include/protstruc_structalign.h: both structures and the DP front live in LDS


def check_structalign_shapes(a, b, mask_a=None, mask_b=None, d0=None) -> Tuple[int, int, int]:
    """Shape rules of ``structure_align``, on shapes, dtypes and devices only (no launch): ValueError.  ``a`` (B,Ma,3) and ``b``
    (B,Mb,3) floating point with ``B <= MAX_BATCH`` and ``1 <= Ma, Mb <= STRUCTALIGN_MAX_POINTS``; ``mask_a`` (B,Ma), ``mask_b``
    (B,Mb); ``d0`` (B,) floating point.  Returns (B, Ma, Mb)."""
    for name, x in (("a", a), ("b", b)):
        M = _float_dims(x, name, "batch, points, 3")[1]
        if not 1 <= M <= STRUCTALIGN_MAX_POINTS:   # names the operand: not _check_count's words
            raise ValueError(f"1 .. {STRUCTALIGN_MAX_POINTS} points per structure, got {M} in {name}")
    B, Ma, Mb = a.shape[0], a.shape[1], b.shape[1]
    _check_batch(B)
    if b.shape[0] != B:
        raise ValueError(f"b must have the batch size of a, {B}, got {b.shape[0]}")
    _check_optional(mask_a, (B, Ma), "mask_a", "a", tuple(a.shape))
    _check_optional(mask_b, (B, Mb), "mask_b", "b", tuple(b.shape))
    _check_optional(d0, (B,), "d0", "a", tuple(a.shape), floating=True)
    _same_device(a, b=b, mask_a=mask_a, mask_b=mask_b, d0=d0)
    return B, Ma, Mb


def _structalign_workspace(B: int, Ma: int, Mb: int, device) -> torch.Tensor:
    return torch.empty(_lib.load().ps_structalign_workspace_bytes(B, Ma, Mb), dtype=torch.uint8, device=device)


def check_nw_align_shapes(score, gap, mask_a=None, mask_b=None) -> Tuple[int, int, int]:
    """Shape rules of ``nw_align``, on shapes, dtypes, devices and the scalar only (no launch): ValueError.  ``score``
    (B,Ma,Mb) floating point with ``B <= MAX_BATCH`` and ``1 <= Ma, Mb <= STRUCTALIGN_MAX_POINTS``; ``gap <= 0`` and finite;
    ``mask_a`` (B,Ma), ``mask_b`` (B,Mb).  Returns (B, Ma, Mb)."""
    shape = _float_dims(score, "score", "batch, rows, columns", tail=())
    B, Ma, Mb = shape
    _check_batch(B)
    if not (1 <= Ma <= STRUCTALIGN_MAX_POINTS and 1 <= Mb <= STRUCTALIGN_MAX_POINTS):
        raise ValueError(f"1 .. {STRUCTALIGN_MAX_POINTS} rows and columns, got {Ma} x {Mb}")
    if not -_INF < float(gap) <= 0:
        raise ValueError(f"gap must be <= 0 and finite, got {gap}")
    _check_optional(mask_a, (B, Ma), "mask_a", "score", shape)
    _check_optional(mask_b, (B, Mb), "mask_b", "score", shape)
    _same_device(score, mask_a=mask_a, mask_b=mask_b)
    return shape


def nw_align(score: torch.Tensor, gap: float, mask_a: Optional[torch.Tensor] = None, mask_b: Optional[torch.Tensor] = None):
    """K41.  One Needleman-Wunsch pass with TM-align's gap rule over ``score`` (B,Ma,Mb) -- the gap penalty ``gap <= 0`` is
    charged only for leaving an aligned pair --: ``(map (B,Ma) int32, n_aligned (B,) int32, value (B,) fp32)``.  The rows
    and columns are the slots with ``mask_a`` (B,Ma) and ``mask_b`` (B,Mb) set (None = all); ``map`` holds for a slot of the
    rows the slot of the columns aligned to it, or -1, and ``value`` the DP's corner value.  Scores at masked slots are never
    read.  The recurrence, its ties and the trace back are defined bit for bit in include/protstruc_structalign.h; the
    table is double.  ``Ma, Mb <= STRUCTALIGN_MAX_POINTS``."""
    B, Ma, Mb = check_nw_align_shapes(score, gap, mask_a, mask_b)
    x, ma, mb = _f32c(score, "score"), _u8c(mask_a, "mask_a"), _u8c(mask_b, "mask_b")
    dev = x.device
    with _on(dev):
        out = torch.empty(B, Ma, dtype=torch.int32, device=dev)           # the kernel writes every element
        n_aligned = torch.empty(B, dtype=torch.int32, device=dev)
        value = torch.empty(B, dtype=torch.float32, device=dev)
        if B:
            workspace = _structalign_workspace(B, Ma, Mb, dev)
            _launch("ps_nw_align_f32", _ptr(x), _ptr(ma), _ptr(mb), float(gap), _ptr(workspace), _ptr(out), _ptr(n_aligned), _ptr(value),
                    B, Ma, Mb, _stream(x))
    return out, n_aligned, value


def check_ca_secondary_structure_shapes(points, mask=None) -> Tuple[int, int]:
    """Shape rules of ``ca_secondary_structure``, on shapes, dtypes and devices only (no launch): ValueError.  ``points``
    (B,M,3) floating point with ``B <= MAX_BATCH`` and ``1 <= M <= STRUCTALIGN_MAX_POINTS``; ``mask`` (B,M).  Returns (B, M)."""
    B, M = _points_dims(points, STRUCTALIGN_MAX_POINTS)
    _check_count(M, 1, STRUCTALIGN_MAX_POINTS, "points per structure")
    _check_optional(mask, (B, M), "mask", "points", tuple(points.shape))
    _same_device(points, mask=mask)
    return B, M


def ca_secondary_structure(points: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K44.  TM-align's secondary structure of CA traces ``points`` (B,M,3): (B,M) int8 -- 1 helix, 2 strand, 3 turn, 0
    anything else and the two points at either end, -1 under ``mask`` (B,M; None = all) -- from the six distances among
    the points i-2 .. i+2 counted after masking.  Chain breaks are not looked at (include/protstruc_structalign.h).
    ``M <= STRUCTALIGN_MAX_POINTS``."""
    B, M = check_ca_secondary_structure_shapes(points, mask)
    x, m = _f32c(points, "points"), _u8c(mask, "mask")
    dev = x.device
    with _on(dev):
        labels = torch.empty(B, M, dtype=torch.int8, device=dev)          # the kernel writes every element
        if B:
            _launch("ps_ca_secondary_structure_f32", _ptr(x), _ptr(m), _ptr(labels), B, M, _stream(x))
    return labels


def structure_align(a: torch.Tensor, b: torch.Tensor, mask_a: Optional[torch.Tensor], mask_b: Optional[torch.Tensor],
                    d0: torch.Tensor, use_secondary_structure: bool = True):
    """K42 / K43.  The alignment of ``a`` (B,Ma,3) onto ``b`` (B,Mb,3) without a given correspondence: ``(map (B,Ma) int32,
    n_aligned (B,) int32, score (B,) fp32, R (B,3,3), t (B,3), n_points (B,2) int32, start (B,) int32)``.  The points are the
    slots with ``mask_a`` / ``mask_b`` set (None = all; entries under a mask are never read); ``map`` holds for a slot of ``a``
    the slot of ``b`` aligned to it, or -1; ``score`` is the best ``sum 1 / (1 + d^2 / d0^2)`` over the aligned pairs divided by
    ``min(n_a, n_b)``, with the transform ``R a + t`` that attains it; ``start`` says which start gave it (0 threading, 1
    secondary structure).  ``d0`` (B,) is positive and finite.  Two starts, each refined by alternating a Needleman-Wunsch
    pass over the TM terms with the seeded superposition search of ``superpose_search`` over the aligned pairs, as
    include/protstruc_structalign.h defines it; deterministic, no host read.  ``Ma, Mb <= STRUCTALIGN_MAX_POINTS``.  A pair
    with an empty side gives a map of -1, score 0 and NaN transforms.  Not differentiable."""
    B, Ma, Mb = check_structalign_shapes(a, b, mask_a, mask_b, d0)
    x, y, ma, mb, scale = _f32c(a, "a"), _f32c(b, "b"), _u8c(mask_a, "mask_a"), _u8c(mask_b, "mask_b"), _f32c(d0, "d0")
    dev = x.device
    with _on(dev):
        out = torch.empty(B, Ma, dtype=torch.int32, device=dev)           # the kernels write every element
        n_aligned = torch.empty(B, dtype=torch.int32, device=dev)
        score = torch.empty(B, dtype=torch.float32, device=dev)
        R = torch.empty(B, 3, 3, dtype=torch.float32, device=dev)
        t = torch.empty(B, 3, dtype=torch.float32, device=dev)
        n_points = torch.empty(B, 2, dtype=torch.int32, device=dev)
        start = torch.empty(B, dtype=torch.int32, device=dev)
        if B:
            workspace = _structalign_workspace(B, Ma, Mb, dev)
            _launch("ps_structure_align_f32", _ptr(x), _ptr(ma), _ptr(y), _ptr(mb), _ptr(scale), int(bool(use_secondary_structure)),
                    _ptr(workspace), _ptr(out), _ptr(n_aligned), _ptr(score), _ptr(R), _ptr(t), _ptr(n_points), _ptr(start), B, Ma,
                    Mb, _stream(x))
    return out, n_aligned, score, R, t, n_points, start


CLUSTER_MAX_ITEMS = 4096   # PS_CLUSTER_MAX_ITEMS of include/protstruc_ensemble.h: the degrees of a matrix live in LDS
RMSD_MATRIX_MAX_POINTS = 2 ** 31 - 17   # PS_RMSD_MATRIX_MAX_POINTS: the points are walked in chunks of 16 by an int


def check_rmsd_matrix_shapes(a, b=None, mask_a=None, mask_b=None) -> Tuple[int, int, int]:
    """Shape rules of ``rmsd_matrix``, on shapes, dtypes and devices only (no launch): ValueError.  ``a`` (Ba,M,3) floating
    point with ``Ba <= MAX_BATCH`` and ``1 <= M <= RMSD_MATRIX_MAX_POINTS``; ``b`` (Bb,M,3) likewise, or None -- self mode, ``a`` against itself, which takes
    no ``mask_b``; ``mask_a`` (Ba,M) and ``mask_b`` (Bb,M).  Returns (Ba, Bb, M)."""
    shape = _float_dims(a, "a", "batch, points, 3")
    Ba, M = shape[:2]
    _check_count(M, 1, RMSD_MATRIX_MAX_POINTS, "points per structure")
    Bb = Ba
    if b is None:
        if mask_b is not None:
            raise ValueError("mask_b needs a b: in self mode (b None) mask_a serves both sides")
    else:
        if len(tuple(b.shape)) != 3 or tuple(b.shape[1:]) != (M, 3):
            raise ValueError(f"b must have shape (batch, {M}, 3) to match a {shape}, got {tuple(b.shape)}")
        if not b.dtype.is_floating_point:
            raise ValueError(f"b must be a floating-point tensor, got {b.dtype}")
        Bb = b.shape[0]
    _check_batch(max(Ba, Bb))
    _check_optional(mask_a, (Ba, M), "mask_a", "a", shape)
    if b is not None:
        _check_optional(mask_b, (Bb, M), "mask_b", "b", tuple(b.shape))
    _same_device(a, b=b, mask_a=mask_a, mask_b=mask_b)
    return Ba, Bb, M


def rmsd_matrix(a: torch.Tensor, b: Optional[torch.Tensor] = None, mask_a: Optional[torch.Tensor] = None,
                mask_b: Optional[torch.Tensor] = None, return_count: bool = False):
    """K45.  The RMSD after optimal superposition of every structure of ``a`` (Ba,M,3) against every structure of ``b``
    (Bb,M,3): (Ba,Bb) fp32, and with ``return_count`` the number of points each pair has in common, (Ba,Bb) int32.  ``b`` None
    is self mode: ``a`` against itself, only the tiles on and above the diagonal computed, both planes exactly symmetric and
    the diagonal exactly 0.  The points of a pair are those that ``mask_a`` (Ba,M) and ``mask_b`` (Bb,M) both count (None =
    all); a pair without any is NaN, and NaN under a structure's own mask reaches nothing.  One tiled double-precision HIP
    kernel over the five sums of a pair, the 3x3 solve of ``kabsch`` as its epilogue; no atomics, and a sub-batch gives the
    block of the full matrix bit for bit.  The RMSD of identical members is NOT 0 but about 1e-6 A (the formula is
    ``E0 - 2 tr``; include/protstruc_ensemble.h states the bound) -- ``superpose`` remains the tool when that matters."""
    Ba, Bb, M = check_rmsd_matrix_shapes(a, b, mask_a, mask_b)
    x, y, ma, mb = _f32c(a, "a"), _f32c_opt(b, "b"), _u8c(mask_a, "mask_a"), _u8c(mask_b, "mask_b")
    dev = x.device
    with _on(dev):
        rmsd = torch.empty(Ba, Bb, dtype=torch.float32, device=dev)       # the kernel writes every element
        count = torch.empty(Ba, Bb, dtype=torch.int32, device=dev) if return_count else None
        if Ba and Bb:   # an empty tensor has no device pointer, and NULL for b means self mode
            _launch("ps_rmsd_matrix_f32", _ptr(x), _ptr(ma), _ptr(y), _ptr(mb), _ptr(rmsd), _ptr(count), Ba, Bb, M, _stream(x))
    return (rmsd, count) if return_count else rmsd


def check_cluster_shapes(D, cutoff, valid=None) -> Tuple[int, int]:
    """Shape rules of ``cluster``, on shapes, dtypes and devices only (no launch): ValueError.  ``D`` (G,B,B) floating point
    with ``G <= MAX_BATCH`` and ``1 <= B <= CLUSTER_MAX_ITEMS``; ``cutoff`` a finite number; ``valid`` (G,B).  Returns (G, B)."""
    shape = tuple(D.shape)
    if len(shape) != 3 or shape[1] != shape[2]:
        raise ValueError(f"D must have shape (matrices, items, items), got {shape}")
    if not D.dtype.is_floating_point:
        raise ValueError(f"D must be a floating-point tensor, got {D.dtype}")
    G, B = shape[:2]
    _check_batch(G, "matrices")
    _check_count(B, 1, CLUSTER_MAX_ITEMS, "items per matrix")
    _check_scalar(cutoff, "cutoff", "finite")
    _check_optional(valid, (G, B), "valid", "D", shape)
    _same_device(D, valid=valid)
    return G, B


def cluster(D: torch.Tensor, cutoff: float, valid: Optional[torch.Tensor] = None):
    """K46.  Clustering of the distance matrices ``D`` (G,B,B) by ``cutoff`` after Daura et al. ("gromos"): ``(label (G,B),
    center (G,B), size (G,B), n_clusters (G,))`` int32.  Two items are neighbours where ``D[min(i,j), max(i,j)] <= cutoff`` --
    only the upper triangle is read, NaN is no neighbour --; among the items still active (at first those of ``valid``
    (G,B), None = all) the one with the most active neighbours, the lowest index on ties, becomes the centre of the next
    cluster and leaves with its active neighbours, until none is left.  ``label`` is -1 at invalid items; ``center`` and
    ``size`` are indexed by cluster number, -1 and 0 from ``n_clusters`` on; sizes never increase.  Integer work, defined bit
    for bit (include/protstruc_ensemble.h); two launches, no host read.  ``B <= CLUSTER_MAX_ITEMS``."""
    G, B = check_cluster_shapes(D, cutoff, valid)
    x, v = _f32c(D, "D"), _u8c(valid, "valid")
    dev = x.device
    with _on(dev):
        label = torch.empty(G, B, dtype=torch.int32, device=dev)          # the kernels write every element
        center = torch.empty(G, B, dtype=torch.int32, device=dev)
        size = torch.empty(G, B, dtype=torch.int32, device=dev)
        n_clusters = torch.empty(G, dtype=torch.int32, device=dev)
        if G:
            workspace = torch.empty(_lib.load().ps_cluster_workspace_bytes(G, B), dtype=torch.uint8, device=dev)
            _launch("ps_cluster_f32", _ptr(x), _ptr(v), float(cutoff), _ptr(workspace), _ptr(label), _ptr(center), _ptr(size),
                    _ptr(n_clusters), G, B, _stream(x))
    return label, center, size, n_clusters


EDGE_MAX_PAIRS = 64  # PS_EDGE_MAX_PAIRS of include/protstruc_hip.h: a residue's k * P distances live in LDS
EDGE_MAX_RBF = 64     # PS_EDGE_MAX_RBF: the centres travel in the kernel's arguments


def _check_neighbor_idx(idx, B: int, N: int, like: str) -> int:
    """k of the neighbour lists ``idx`` (B,N,k) of ``nearest_neighbors`` on the N axis of ``like``; ValueError otherwise."""
    shape = tuple(idx.shape)
    if len(shape) != 3 or shape[:2] != (B, N):
        raise ValueError(f"idx must have shape ({B}, {N}, k) to match {like}, got {shape}")
    if not _is_integer_tensor(idx):
        raise ValueError(f"idx must be an integer tensor, got {idx.dtype}")
    if not 1 <= shape[2] <= KNN_MAX_K:
        raise ValueError(f"idx must hold 1 .. {KNN_MAX_K} neighbours per residue, got {shape[2]}")
    return shape[2]


def _idx32(idx: torch.Tensor, N: int) -> torch.Tensor:
    """``idx`` as contiguous int32 for the edge kernels, to which every value outside [0, N) is padding: wider integers
    are clamped to [-1, N] first, so that none wraps into the range."""
    _require_device(idx, "idx")
    if idx.dtype != torch.int32:
        idx = idx.clamp(-1, N).to(torch.int32)
    return idx.contiguous()


def _host_f32(values, name: str) -> np.ndarray:
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().numpy()
    try:
        arr = np.asarray(values, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a sequence of numbers") from None
    if arr.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional, got shape {arr.shape}")
    return arr


def check_edge_rbf_shapes(xyz, idx, atom_mask=None, pair_i=(), pair_j=(), centers=(), sigma=1.0, want_dist=True,
                          want_rbf=True) -> None:
    """Shape rules of ``edge_rbf``, on shapes, dtypes, devices, the host tables and the scalar only (no launch):
    ValueError.  ``idx`` (B,N,k) integers with ``1 <= k <= KNN_MAX_K``; ``pair_i`` and ``pair_j`` equally long, 1 ..
    ``EDGE_MAX_PAIRS`` atom slots in [0, A); 1 .. ``EDGE_MAX_RBF`` ``centers``; ``sigma`` positive and finite; one of
    the two outputs wanted."""
    B, N, A = _xyz_dims(xyz)
    _check_batch(B)
    _check_count(N, 0, 2 ** 24, "residues per structure")
    _check_neighbor_idx(idx, B, N, f"xyz {(B, N, A, 3)}")
    _check_optional(atom_mask, (B, N, A), "atom_mask", "xyz", (B, N, A, 3))
    try:
        slots_i, slots_j = [int(s) for s in pair_i], [int(s) for s in pair_j]
    except (TypeError, ValueError):
        raise ValueError("pair_i and pair_j must be sequences of atom slots") from None
    if len(slots_i) != len(slots_j) or not 1 <= len(slots_i) <= EDGE_MAX_PAIRS:
        raise ValueError(f"pair_i and pair_j must be equally long, 1 .. {EDGE_MAX_PAIRS} atom slots each, got "
                         f"{len(slots_i)} and {len(slots_j)}")
    _check_atom_slots(A, *slots_i, *slots_j)
    R = _host_f32(centers, "centers").shape[0]
    if not 1 <= R <= EDGE_MAX_RBF:
        raise ValueError(f"centers must hold 1 .. {EDGE_MAX_RBF} values, got {R}")
    _check_scalar(sigma, "sigma", "positive")
    if not (want_dist or want_rbf):
        raise ValueError("nothing to compute: want_dist and want_rbf are both False")
    _same_device(xyz, idx=idx, atom_mask=atom_mask)


def edge_rbf(xyz: torch.Tensor, idx: torch.Tensor, atom_mask: Optional[torch.Tensor] = None, *, pair_i: Sequence[int],
             pair_j: Sequence[int], centers, sigma: float, want_dist: bool = True, want_rbf: bool = True):
    """K25.  Radial basis functions of the atom-pair distances along the edges of a neighbour graph, fused: ``(dist
    (B,N,k,P) fp32, rbf (B,N,k,P*R) fp32)``, None for an output not wanted.  ``xyz`` (B,N,A,3); ``idx`` (B,N,k) the
    neighbour lists of ``nearest_neighbors`` on the same N axis -- any entry outside [0, N) is padding --; pair p is atom
    slot ``pair_i[p]`` of the source residue against slot ``pair_j[p]`` of the neighbour; ``centers`` are R values.
    ``dist = sqrt((dx*dx + dy*dy) + dz*dz)`` in double on the float32 inputs, rounded once (K24's distance, defined bit
    for bit); ``rbf[..., p*R + c] = exp(-((dist - centers[c]) / sigma)^2)`` in float32, within 1e-6 absolute of the
    float64 value.  Both are exactly 0 at the padding and where either atom is outside ``atom_mask`` (B,N,A; None =
    all); NaN under the mask never reaches arithmetic.  Nothing of the size of the gathered coordinates or of a
    broadcast intermediate is built; every element is written; deterministic (include/protstruc_hip.h)."""
    check_edge_rbf_shapes(xyz, idx, atom_mask, pair_i, pair_j, centers, sigma, want_dist, want_rbf)
    x, am = _f32c(xyz, "xyz"), _u8c(atom_mask, "atom_mask")
    B, N, A = x.shape[:3]
    nb = _idx32(idx, N)
    k = nb.shape[2]
    cen = _host_f32(centers, "centers")
    P, R = len(pair_i), cen.shape[0]
    ints = ctypes.c_int * P
    with _on(x.device):
        # the kernel writes every element; an empty tensor has no device pointer and nothing is launched for it
        dist = torch.empty(B, N, k, P, dtype=torch.float32, device=x.device) if want_dist else None
        rbf = torch.empty(B, N, k, P * R, dtype=torch.float32, device=x.device) if want_rbf else None
        if B and N:
            _launch("ps_edge_rbf_f32", _ptr(x), _ptr(am), _ptr(nb), ints(*(int(s) for s in pair_i)),
                    ints(*(int(s) for s in pair_j)), P, (ctypes.c_float * R)(*cen.tolist()), R, float(sigma), _ptr(dist),
                    _ptr(rbf), B, N, A, k, _stream(x))
    return dist, rbf


def check_edge_frames_shapes(rot, trans, idx, frame_mask=None, want_pos=True, want_rot=True) -> None:
    """Shape rules of ``edge_frames``, on shapes, dtypes and devices only (no launch): ValueError."""
    shape = _float_dims(rot, "rot", "batch, frames, 3, 3", tail=(3, 3))
    B, N = shape[:2]
    _check_batch(B)
    _check_count(N, 0, 2 ** 24, "frames per structure")
    _check_float_tensor(trans, (B, N, 3), "trans", f"rot {shape}")
    _check_neighbor_idx(idx, B, N, f"rot {shape}")
    _check_optional(frame_mask, (B, N), "frame_mask", "rot", shape)
    if not (want_pos or want_rot):
        raise ValueError("nothing to compute: want_pos and want_rot are both False")
    _same_device(rot, trans=trans, idx=idx, frame_mask=frame_mask)


def edge_frames(rot: torch.Tensor, trans: torch.Tensor, idx: torch.Tensor, frame_mask: Optional[torch.Tensor] = None, *,
                want_pos: bool = True, want_rot: bool = True):
    """K26.  The neighbour's frame in the source residue's frame along the edges of a neighbour graph: ``(local_pos
    (B,N,k,3), rel_rot (B,N,k,3,3))`` fp32, None for an output not wanted.  ``rot`` (B,N,3,3) has the basis vectors as
    columns, as ``frames`` returns it, ``trans`` is (B,N,3); ``idx`` (B,N,k) as for ``edge_rbf``.  ``local_pos = R_i^T
    (t_j - t_i)`` and ``rel_rot = R_i^T R_j``, evaluated in double on the float32 inputs in the order stated in
    include/protstruc_hip.h and rounded once: defined bit for bit.  Exactly 0 at the padding and where i or j is outside
    ``frame_mask`` (B,N; None = all); frames there are never read.  Every element is written; deterministic."""
    check_edge_frames_shapes(rot, trans, idx, frame_mask, want_pos, want_rot)
    r, t, fm = _f32c(rot, "rot"), _f32c(trans, "trans"), _u8c(frame_mask, "frame_mask")
    B, N = r.shape[:2]
    nb = _idx32(idx, N)
    k = nb.shape[2]
    with _on(r.device):
        pos = torch.empty(B, N, k, 3, dtype=torch.float32, device=r.device) if want_pos else None
        rel = torch.empty(B, N, k, 3, 3, dtype=torch.float32, device=r.device) if want_rot else None
        if B and N:
            _launch("ps_edge_frames_f32", _ptr(r), _ptr(t), _ptr(fm), _ptr(nb), _ptr(pos), _ptr(rel), B, N, k, _stream(r))
    return pos, rel


CSREDGE_CHUNK = 64   # PS_CSREDGE_CHUNK of include/protstruc_csredge.h
CSREDGE_MAX_PAIRS = 64   # PS_CSREDGE_MAX_PAIRS: a chunk's 64 * P distances live in LDS
CSREDGE_MAX_RBF = 64   # PS_CSREDGE_MAX_RBF: the centres travel in the kernel's arguments


def _launch_csredge(name: str, *args) -> None:
    """Call entry point ``name`` of libprotstruc_csredge.so; HipLibraryError if it does not return hipSuccess."""
    rc = getattr(_csredge.load(), name)(*args)
    if rc:
        _csredge.check(rc, name)


def _check_csr_graph(row_ptr, col, B: int, Q: int, like: str) -> int:
    """E, the length of the edge buffers of the CSR lists ``row_ptr`` (B*Q+1,), ``col`` (E,) over the B x Q sources of
    ``like``; ValueError otherwise."""
    if tuple(row_ptr.shape) != (B * Q + 1,):
        raise ValueError(f"row_ptr must have shape ({B * Q + 1},) to match the {B} x {Q} sources of {like}, "
                         f"got {tuple(row_ptr.shape)}")
    if not _is_integer_tensor(row_ptr):
        raise ValueError(f"row_ptr must be an integer tensor, got {row_ptr.dtype}")
    if col.ndim != 1:
        raise ValueError(f"col must have shape (edges,), got {tuple(col.shape)}")
    if not _is_integer_tensor(col):
        raise ValueError(f"col must be an integer tensor, got {col.dtype}")
    return col.shape[0]


def _row_ptr64(row_ptr: torch.Tensor) -> torch.Tensor:
    _require_device(row_ptr, "row_ptr")
    return (row_ptr if row_ptr.dtype == torch.int64 else row_ptr.to(torch.int64)).contiguous()


def _col32(col: torch.Tensor, M: int) -> torch.Tensor:
    """``col`` as contiguous int32 for the CSR edge kernels, to which every value outside [0, M) is padding: wider integers
    are clamped to [-1, M] first, so that none wraps into the range."""
    _require_device(col, "col")
    if col.dtype != torch.int32:
        col = col.clamp(-1, M).to(torch.int32)
    return col.contiguous()


def check_csr_edge_rows_shapes(row_ptr, Q, E) -> int:
    """Shape rules of ``csr_edge_rows`` (no launch): ValueError; returns B.  ``row_ptr`` (B*Q+1,) integers; ``Q`` an integer
    in 0 .. 2^24 that divides the number of rows; ``E`` a non-negative integer."""
    for name, value in (("Q", Q), ("E", E)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 0:
            raise ValueError(f"{name} must be a non-negative integer, got {value!r}")
    _check_count(int(Q), 0, 2 ** 24, "queries per structure")
    if row_ptr.ndim != 1 or row_ptr.shape[0] < 1:
        raise ValueError(f"row_ptr must have shape (rows + 1,), got {tuple(row_ptr.shape)}")
    if not _is_integer_tensor(row_ptr):
        raise ValueError(f"row_ptr must be an integer tensor, got {row_ptr.dtype}")
    rows = row_ptr.shape[0] - 1
    if rows % Q if Q else rows:
        raise ValueError(f"row_ptr holds {rows} rows, no multiple of Q = {Q}")
    B = rows // Q if Q else 0
    _check_batch(B)
    return B


def csr_edge_rows(row_ptr: torch.Tensor, Q: int, E: int):
    """K49.  ``(batch (E,) int32, row (E,) int32)``: the structure and the query of every edge position of CSR lists
    ``row_ptr`` (B*Q+1,) whose edge buffers hold ``E`` entries -- ``col.shape[0]``, not ``row_ptr[-1]`` --, both -1 at the
    positions from ``row_ptr[-1]`` on.  Position p belongs to the row r with ``row_ptr[r] <= p < row_ptr[r + 1]``, found on
    the device by bisection: the triples of ``geometry.radius_graph_edges`` without its host read, so it runs inside a
    captured graph (include/protstruc_csredge.h)."""
    check_csr_edge_rows_shapes(row_ptr, Q, E)
    rp = _row_ptr64(row_ptr)
    Q, E = int(Q), int(E)
    with _on(rp.device):
        if not E:   # nothing to launch (an empty tensor has no device pointer)
            return (torch.empty(0, dtype=torch.int32, device=rp.device), torch.empty(0, dtype=torch.int32, device=rp.device))
        batch = torch.empty(E, dtype=torch.int32, device=rp.device)   # the kernel writes every element
        row = torch.empty(E, dtype=torch.int32, device=rp.device)
        _launch_csredge("ps_csr_edge_rows_i32", _ptr(rp), rp.shape[0] - 1, Q, E, _ptr(batch), _ptr(row), _stream(rp))
    return batch, row


def check_csr_edge_rbf_shapes(xyz, row_ptr, col, atom_mask=None, pair_i=(), pair_j=(), centers=(), sigma=1.0, src_xyz=None,
                              src_mask=None, want_dist=True, want_rbf=True) -> Tuple[int, int, int, int, int, int]:
    """Shape rules of ``csr_edge_rbf``, on shapes, dtypes, devices, the host tables and the scalar only (no launch):
    ValueError; returns (B, M, A, Q, As, E).  ``xyz`` (B,M,A,3) the targets; ``src_xyz`` (B,Q,As,3) the sources or None,
    the targets, which takes no ``src_mask``; ``row_ptr`` (B*Q+1,) and ``col`` (E,) integers; ``pair_i`` slots in [0, As),
    ``pair_j`` in [0, A), equally long, 1 .. ``CSREDGE_MAX_PAIRS``; 1 .. ``CSREDGE_MAX_RBF`` ``centers``; ``sigma`` positive
    and finite; one of the two outputs wanted."""
    B, M, A = _xyz_dims(xyz)
    _check_batch(B)
    _check_count(M, 0, 2 ** 24, "residues per structure")
    _check_optional(atom_mask, (B, M, A), "atom_mask", "xyz", (B, M, A, 3))
    Q, As = M, A
    if src_xyz is None:
        if src_mask is not None:
            raise ValueError("src_mask needs src_xyz: where the sources are the targets, atom_mask is used")
    else:
        shape = tuple(src_xyz.shape)
        if len(shape) != 4 or shape[3] != 3 or shape[0] != B:
            raise ValueError(f"src_xyz must have shape ({B}, queries, atoms, 3) to match xyz {(B, M, A, 3)}, got {shape}")
        if not src_xyz.dtype.is_floating_point:
            raise ValueError(f"src_xyz must be a floating-point tensor, got {src_xyz.dtype}")
        Q, As = shape[1:3]
        _check_count(Q, 0, 2 ** 24, "queries per structure")
        _check_optional(src_mask, (B, Q, As), "src_mask", "src_xyz", shape)
    E = _check_csr_graph(row_ptr, col, B, Q, f"xyz {(B, M, A, 3)}" if src_xyz is None else f"src_xyz {tuple(src_xyz.shape)}")
    try:
        slots_i, slots_j = [int(s) for s in pair_i], [int(s) for s in pair_j]
    except (TypeError, ValueError):
        raise ValueError("pair_i and pair_j must be sequences of atom slots") from None
    if len(slots_i) != len(slots_j) or not 1 <= len(slots_i) <= CSREDGE_MAX_PAIRS:
        raise ValueError(f"pair_i and pair_j must be equally long, 1 .. {CSREDGE_MAX_PAIRS} atom slots each, got "
                         f"{len(slots_i)} and {len(slots_j)}")
    _check_atom_slots(As, *slots_i)
    _check_atom_slots(A, *slots_j)
    R = _host_f32(centers, "centers").shape[0]
    if not 1 <= R <= CSREDGE_MAX_RBF:
        raise ValueError(f"centers must hold 1 .. {CSREDGE_MAX_RBF} values, got {R}")
    _check_scalar(sigma, "sigma", "positive")
    if not (want_dist or want_rbf):
        raise ValueError("nothing to compute: want_dist and want_rbf are both False")
    _same_device(xyz, row_ptr=row_ptr, col=col, atom_mask=atom_mask, src_xyz=src_xyz, src_mask=src_mask)
    return B, M, A, Q, As, E


def csr_edge_rbf(xyz: torch.Tensor, row_ptr: torch.Tensor, col: torch.Tensor, atom_mask: Optional[torch.Tensor] = None, *,
                 pair_i: Sequence[int], pair_j: Sequence[int], centers, sigma: float, src_xyz: Optional[torch.Tensor] = None,
                 src_mask: Optional[torch.Tensor] = None, want_dist: bool = True, want_rbf: bool = True):
    """K50.  ``edge_rbf`` on CSR lists of any length: ``(dist (E,P) fp32, rbf (E,P*R) fp32)``, None for an output not wanted,
    one row per edge position.  ``xyz`` (B,M,A,3) are the targets, what ``col`` (E,) indexes; ``src_xyz`` (B,Q,As,3) the
    sources, the rows of ``row_ptr`` (B*Q+1,) -- None: the targets themselves (Q = M), with ``atom_mask`` for both.  Pair p is
    slot ``pair_i[p]`` of the source against slot ``pair_j[p]`` of the target.  The arithmetic is ``edge_rbf``'s, and on
    the same edge so are the bits.  A position is padding from ``row_ptr[-1]`` on and where ``col`` is outside [0, M):
    exactly 0, like a pair with an atom outside its mask, and nothing is read there.  E is ``col.shape[0]``; lists cut by
    ``max_edges`` are served for the positions that exist.  No host read, so capturable; every element is written;
    deterministic (include/protstruc_csredge.h)."""
    B, M, A, Q, As, E = check_csr_edge_rbf_shapes(xyz, row_ptr, col, atom_mask, pair_i, pair_j, centers, sigma, src_xyz, src_mask,
                                                  want_dist, want_rbf)
    x, am = _f32c(xyz, "xyz"), _u8c(atom_mask, "atom_mask")
    sx, sm = _f32c_opt(src_xyz, "src_xyz"), _u8c(src_mask, "src_mask")
    rp, cl = _row_ptr64(row_ptr), _col32(col, M)
    cen = _host_f32(centers, "centers")
    P, R = len(pair_i), cen.shape[0]
    ints = ctypes.c_int * P
    with _on(x.device):
        if not (B and E and M and Q):   # nothing to launch (an empty tensor has no device pointer): all padding
            return (torch.zeros(E, P, dtype=torch.float32, device=x.device) if want_dist else None,
                    torch.zeros(E, P * R, dtype=torch.float32, device=x.device) if want_rbf else None)
        dist = torch.empty(E, P, dtype=torch.float32, device=x.device) if want_dist else None   # every element is written
        rbf = torch.empty(E, P * R, dtype=torch.float32, device=x.device) if want_rbf else None
        _launch_csredge("ps_csr_edge_rbf_f32", _ptr(x), _ptr(am), _ptr(sx), _ptr(sm), _ptr(rp), _ptr(cl), E,
                        ints(*(int(s) for s in pair_i)), ints(*(int(s) for s in pair_j)), P, (ctypes.c_float * R)(*cen.tolist()),
                        R, float(sigma), _ptr(dist), _ptr(rbf), B, M, A, Q, As, _stream(x))
    return dist, rbf


def check_csr_edge_frames_shapes(rot, trans, row_ptr, col, frame_mask=None, src_rot=None, src_trans=None, src_mask=None,
                                 want_pos=True, want_rot=True) -> Tuple[int, int, int, int]:
    """Shape rules of ``csr_edge_frames``, on shapes, dtypes and devices only (no launch): ValueError; returns (B, M, Q, E)."""
    shape = _float_dims(rot, "rot", "batch, frames, 3, 3", tail=(3, 3))
    B, M = shape[:2]
    _check_batch(B)
    _check_count(M, 0, 2 ** 24, "frames per structure")
    _check_float_tensor(trans, (B, M, 3), "trans", f"rot {shape}")
    _check_optional(frame_mask, (B, M), "frame_mask", "rot", shape)
    Q = M
    if (src_rot is None) != (src_trans is None):
        raise ValueError("src_rot and src_trans come together: the sources' frames")
    if src_rot is None:
        if src_mask is not None:
            raise ValueError("src_mask needs src_rot and src_trans: where the sources are the targets, frame_mask is used")
    else:
        src_shape = tuple(src_rot.shape)
        if len(src_shape) != 4 or src_shape[2:] != (3, 3) or src_shape[0] != B:
            raise ValueError(f"src_rot must have shape ({B}, queries, 3, 3) to match rot {shape}, got {src_shape}")
        if not src_rot.dtype.is_floating_point:
            raise ValueError(f"src_rot must be a floating-point tensor, got {src_rot.dtype}")
        Q = src_shape[1]
        _check_count(Q, 0, 2 ** 24, "queries per structure")
        _check_float_tensor(src_trans, (B, Q, 3), "src_trans", f"src_rot {src_shape}")
        _check_optional(src_mask, (B, Q), "src_mask", "src_rot", src_shape)
    E = _check_csr_graph(row_ptr, col, B, Q, f"rot {shape}" if src_rot is None else f"src_rot {tuple(src_rot.shape)}")
    if not (want_pos or want_rot):
        raise ValueError("nothing to compute: want_pos and want_rot are both False")
    _same_device(rot, trans=trans, row_ptr=row_ptr, col=col, frame_mask=frame_mask, src_rot=src_rot, src_trans=src_trans,
                 src_mask=src_mask)
    return B, M, Q, E


def csr_edge_frames(rot: torch.Tensor, trans: torch.Tensor, row_ptr: torch.Tensor, col: torch.Tensor,
                    frame_mask: Optional[torch.Tensor] = None, *, src_rot: Optional[torch.Tensor] = None,
                    src_trans: Optional[torch.Tensor] = None, src_mask: Optional[torch.Tensor] = None, want_pos: bool = True,
                    want_rot: bool = True):
    """K51.  ``edge_frames`` on CSR lists of any length: ``(local_pos (E,3), rel_rot (E,3,3))`` fp32, None for an output not
    wanted.  ``rot`` (B,M,3,3), ``trans`` (B,M,3) and ``frame_mask`` (B,M) are the targets' frames, what ``col`` indexes;
    ``src_rot`` (B,Q,3,3), ``src_trans`` (B,Q,3), ``src_mask`` (B,Q) the sources', the rows of ``row_ptr`` -- None: the
    targets themselves.  ``edge_frames``' formulas and, on the same edge, its bits; exactly 0 at the padding (from
    ``row_ptr[-1]`` on, and where ``col`` is outside [0, M)) and where either frame is outside its mask.  No host read;
    every element is written; deterministic (include/protstruc_csredge.h)."""
    B, M, Q, E = check_csr_edge_frames_shapes(rot, trans, row_ptr, col, frame_mask, src_rot, src_trans, src_mask, want_pos, want_rot)
    r, t, fm = _f32c(rot, "rot"), _f32c(trans, "trans"), _u8c(frame_mask, "frame_mask")
    sr, st, sm = _f32c_opt(src_rot, "src_rot"), _f32c_opt(src_trans, "src_trans"), _u8c(src_mask, "src_mask")
    rp, cl = _row_ptr64(row_ptr), _col32(col, M)
    with _on(r.device):
        if not (B and E and M and Q):   # nothing to launch: all padding
            return (torch.zeros(E, 3, dtype=torch.float32, device=r.device) if want_pos else None,
                    torch.zeros(E, 3, 3, dtype=torch.float32, device=r.device) if want_rot else None)
        pos = torch.empty(E, 3, dtype=torch.float32, device=r.device) if want_pos else None
        rel = torch.empty(E, 3, 3, dtype=torch.float32, device=r.device) if want_rot else None
        _launch_csredge("ps_csr_edge_frames_f32", _ptr(r), _ptr(t), _ptr(fm), _ptr(sr), _ptr(st), _ptr(sm), _ptr(rp), _ptr(cl), E,
                        _ptr(pos), _ptr(rel), B, M, Q, _stream(r))
    return pos, rel


# ---- the backward kernels of the edge features (K52 - K54, include/protstruc_edgegrad.h) -------------------------------------
def _launch_edgegrad(name: str, *args) -> None:
    """Call entry point ``name`` of libprotstruc_edgegrad.so; HipLibraryError if it does not return hipSuccess."""
    rc = getattr(_edgegrad.load(), name)(*args)
    if rc:
        _edgegrad.check(rc, name)


def _check_sizes(**sizes) -> None:
    """sizes that arrive as arguments, where other functions read them off a shape: non-negative integers, or ValueError"""
    for name, value in sizes.items():
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 0:
            raise ValueError(f"{name} must be a non-negative integer, got {value!r}")


def _check_incoming(in_ptr, in_edge, B: int, M: int) -> None:
    """The incoming list of ``csr_incoming_edges`` over B x M targets: ``in_ptr`` (B*M+1,) and ``in_edge`` (n,) int64."""
    if tuple(in_ptr.shape) != (B * M + 1,) or in_ptr.dtype != torch.int64:
        raise ValueError(f"in_ptr must be an int64 tensor of shape ({B * M + 1},), the {B} x {M} targets and one, got "
                         f"{in_ptr.dtype} {tuple(in_ptr.shape)}")
    if in_edge.ndim != 1 or in_edge.dtype != torch.int64:
        raise ValueError(f"in_edge must be an int64 tensor of shape (edges,), got {in_edge.dtype} {tuple(in_edge.shape)}")


def csr_incoming_edges(row_ptr: torch.Tensor, col: torch.Tensor, B: int, Q: int, M: int):
    """The transpose's index of CSR lists ``row_ptr`` (B*Q+1,), ``col`` (E,) over B x M targets: ``(ptr (B*M+1,) int64, edge
    (E,) int64)``.  ``edge[ptr[o]:ptr[o + 1]]`` are the edge positions p whose target is ``o = batch(p) * M + col[p]``,
    ascending; the positions that are no edge -- from ``row_ptr[-1]`` on, and wherever ``col`` is outside [0, M) -- belong to
    no group and fill ``edge`` from ``ptr[-1]`` on.  It is what lets a target sum over its edges in a fixed order without
    atomics (``csr_edge_pair_grad_sum``, ``csr_edge_frames_backward``).  Plain torch on the lists' own device, CPU included:
    the row of every position by ``searchsorted``, the key ``batch * M + col`` (``B * M`` for the padding), a stable sort and
    a second ``searchsorted``.  No host read -- no ``bincount``, whose output size is one --, so capturable."""
    _check_sizes(B=B, Q=Q, M=M)
    B, Q, M = int(B), int(Q), int(M)
    _check_batch(B)
    _check_count(Q, 0, 2 ** 24, "queries per structure")
    _check_count(M, 0, 2 ** 24, "points per structure")
    E = _check_csr_graph(row_ptr, col, B, Q, f"{B} structures")
    _same_device(row_ptr, col=col)
    dev = row_ptr.device
    position = torch.arange(E, dtype=torch.int64, device=dev)
    rows = torch.searchsorted(row_ptr[1:].to(torch.int64).contiguous(), position, right=True)   # r(p), B * Q in the tail
    target = col.to(torch.int64)
    real = (rows < B * Q) & (target >= 0) & (target < M)
    key = torch.where(real, torch.div(rows, max(Q, 1), rounding_mode="floor") * M + target, torch.full_like(target, B * M))
    key, edge = torch.sort(key, stable=True)
    ptr = torch.searchsorted(key, torch.arange(B * M + 1, dtype=torch.int64, device=dev))
    return ptr, edge


def check_csr_edge_rbf_backward_shapes(xyz, row_ptr, col, atom_mask=None, pair_i=(), pair_j=(), centers=(), sigma=1.0,
                                       src_xyz=None, src_mask=None, grad_dist=None, grad_rbf=None):
    """Shape rules of ``csr_edge_rbf_backward`` (no launch): those of ``csr_edge_rbf``, and ``grad_dist`` (E,P) and
    ``grad_rbf`` (E,P*R) floating-point, one of them given; ValueError; returns (B, M, A, Q, As, E)."""
    dims = check_csr_edge_rbf_shapes(xyz, row_ptr, col, atom_mask, pair_i, pair_j, centers, sigma, src_xyz, src_mask)
    E, P, R = dims[5], len(pair_i), _host_f32(centers, "centers").shape[0]
    if grad_dist is None and grad_rbf is None:
        raise ValueError("nothing to compute: grad_dist and grad_rbf are both None")
    _check_optional(grad_dist, (E, P), "grad_dist", "the edges and pairs", floating=True)
    _check_optional(grad_rbf, (E, P * R), "grad_rbf", "the edges, pairs and centers", floating=True)
    _same_device(xyz, grad_dist=grad_dist, grad_rbf=grad_rbf)
    return dims


def csr_edge_rbf_backward(xyz: torch.Tensor, row_ptr: torch.Tensor, col: torch.Tensor,
                          atom_mask: Optional[torch.Tensor] = None, *, pair_i: Sequence[int], pair_j: Sequence[int], centers,
                          sigma: float, src_xyz: Optional[torch.Tensor] = None, src_mask: Optional[torch.Tensor] = None,
                          grad_dist: Optional[torch.Tensor] = None, grad_rbf: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K52.  The gradient of ``csr_edge_rbf`` (and of ``edge_rbf``) per edge and atom pair: ``pair_grad`` (E,P,3) fp32, the
    derivative of the loss with respect to the TARGET's atom of pair p of every edge, given ``grad_dist`` (E,P) and / or
    ``grad_rbf`` (E,P*R); the source's atom gets its negative (``csr_edge_pair_grad_sum`` adds both up).  The distance and
    the Gaussians are recomputed as the forward computes them; exactly 0 at the padding, where either atom is outside its
    mask and where the distance is 0 (a self edge: defined as 0, not NaN), and nothing -- no coordinate and no element of the
    incoming gradients -- is read there.  The order of every sum is fixed, so the result does not depend on how ``grad_rbf``
    is aligned, and repeats bit for bit.  No host read; every element is written (include/protstruc_edgegrad.h)."""
    B, M, A, Q, As, E = check_csr_edge_rbf_backward_shapes(xyz, row_ptr, col, atom_mask, pair_i, pair_j, centers, sigma, src_xyz,
                                                           src_mask, grad_dist, grad_rbf)
    x, am = _f32c(xyz, "xyz"), _u8c(atom_mask, "atom_mask")
    sx, sm = _f32c_opt(src_xyz, "src_xyz"), _u8c(src_mask, "src_mask")
    gd, gr = _f32c_opt(grad_dist, "grad_dist"), _f32c_opt(grad_rbf, "grad_rbf")
    rp, cl = _row_ptr64(row_ptr), _col32(col, M)
    cen = _host_f32(centers, "centers")
    P, R = len(pair_i), cen.shape[0]
    ints = ctypes.c_int * P
    with _on(x.device):
        if not (B and E and M and Q):   # nothing to launch (an empty tensor has no device pointer): all padding
            return torch.zeros(E, P, 3, dtype=torch.float32, device=x.device)
        pair_grad = torch.empty(E, P, 3, dtype=torch.float32, device=x.device)   # every element is written
        _launch_edgegrad("ps_csr_edge_rbf_backward_f32", _ptr(x), _ptr(am), _ptr(sx), _ptr(sm), _ptr(rp), _ptr(cl), E,
                         ints(*(int(s) for s in pair_i)), ints(*(int(s) for s in pair_j)), P, (ctypes.c_float * R)(*cen.tolist()),
                         R, float(sigma), _ptr(gd), _ptr(gr), _ptr(pair_grad), B, M, A, Q, As, _stream(x))
    return pair_grad


def check_csr_edge_pair_grad_sum_shapes(pair_grad, row_ptr, in_ptr, in_edge, pair_i=(), pair_j=(), B=0, M=0, A=1, Q=None,
                                        As=None) -> Tuple[int, int, int]:
    """Shape rules of ``csr_edge_pair_grad_sum`` (no launch): ValueError; returns (Q, As, E).  ``pair_grad`` (E,P,3) fp32;
    ``row_ptr`` (B*Q+1,) integers; the incoming list of ``csr_incoming_edges``; ``Q`` and ``As`` come together (the bipartite
    graph) or not at all."""
    _check_sizes(B=B, M=M, A=A)
    if (Q is None) != (As is None):
        raise ValueError("Q and As come together: the sources of a bipartite graph")
    if Q is not None:
        _check_sizes(Q=Q, As=As)
    _check_batch(B)
    _check_count(M, 0, 2 ** 24, "residues per structure")
    Qs, Ass = (M, A) if Q is None else (int(Q), int(As))
    _check_count(Qs, 0, 2 ** 24, "queries per structure")
    try:
        slots_i, slots_j = [int(s) for s in pair_i], [int(s) for s in pair_j]
    except (TypeError, ValueError):
        raise ValueError("pair_i and pair_j must be sequences of atom slots") from None
    if len(slots_i) != len(slots_j) or not 1 <= len(slots_i) <= CSREDGE_MAX_PAIRS:
        raise ValueError(f"pair_i and pair_j must be equally long, 1 .. {CSREDGE_MAX_PAIRS} atom slots each, got "
                         f"{len(slots_i)} and {len(slots_j)}")
    if A < 1 or Ass < 1:
        raise ValueError(f"at least one atom slot, got A = {A} and As = {Ass}")
    _check_atom_slots(Ass, *slots_i)
    _check_atom_slots(A, *slots_j)
    P = len(slots_i)
    if pair_grad.ndim != 3 or tuple(pair_grad.shape[1:]) != (P, 3) or not pair_grad.dtype.is_floating_point:
        raise ValueError(f"pair_grad must be a floating-point tensor of shape (edges, {P}, 3), got {pair_grad.dtype} "
                         f"{tuple(pair_grad.shape)}")
    if tuple(row_ptr.shape) != (B * Qs + 1,) or not _is_integer_tensor(row_ptr):
        raise ValueError(f"row_ptr must be an integer tensor of shape ({B * Qs + 1},), the {B} x {Qs} sources and one, got "
                         f"{row_ptr.dtype} {tuple(row_ptr.shape)}")
    _check_incoming(in_ptr, in_edge, B, M)
    _same_device(pair_grad, row_ptr=row_ptr, in_ptr=in_ptr, in_edge=in_edge)
    return Qs, Ass, pair_grad.shape[0]


def csr_edge_pair_grad_sum(pair_grad: torch.Tensor, row_ptr: torch.Tensor, in_ptr: torch.Tensor, in_edge: torch.Tensor, *,
                           pair_i: Sequence[int], pair_j: Sequence[int], B: int, M: int, A: int, Q: Optional[int] = None,
                           As: Optional[int] = None):
    """K53.  The segmented sum of ``pair_grad`` (E,P,3) of ``csr_edge_rbf_backward`` into the gradient of the coordinates:
    ``grad`` (B,M,A,3) fp32 or, with ``Q`` and ``As`` (a bipartite graph), ``(grad, grad_src (B,Q,As,3))``.  Every atom sums,
    in double from +0 and in a fixed order -- its residue's outgoing edge positions ascending, each SUBTRACTED at slot
    ``pair_i[t]``, then the incoming ones of ``csr_incoming_edges`` ascending, each ADDED at slot ``pair_j[t]`` -- and rounds
    once; in a bipartite graph ``grad_src`` takes the first loop and ``grad`` the second.  No atomics; exact +0 for a slot no
    pair names and for a residue without edges; every element is written; no host read (include/protstruc_edgegrad.h)."""
    Qs, Ass, E = check_csr_edge_pair_grad_sum_shapes(pair_grad, row_ptr, in_ptr, in_edge, pair_i, pair_j, B, M, A, Q, As)
    B, M, A = int(B), int(M), int(A)
    pg = _f32c(pair_grad, "pair_grad")
    rp, ip, ie = _row_ptr64(row_ptr), in_ptr.contiguous(), in_edge.contiguous()
    P = len(pair_i)
    ints = ctypes.c_int * P
    with _on(pg.device):
        edges = bool(B and E and M and Qs)   # otherwise nothing is an edge, and an empty tensor has no device pointer
        new = torch.empty if edges else torch.zeros   # the kernel writes every element
        grad = new(B, M, A, 3, dtype=torch.float32, device=pg.device)
        grad_src = None if Q is None else new(B, Qs, Ass, 3, dtype=torch.float32, device=pg.device)
        if edges:
            _launch_edgegrad("ps_csr_edge_pair_grad_sum_f32", _ptr(pg), _ptr(rp), E, _ptr(ip), _ptr(ie), ie.shape[0],
                             ints(*(int(s) for s in pair_i)), ints(*(int(s) for s in pair_j)), P, _ptr(grad), _ptr(grad_src),
                             B, M, A, Qs, Ass, _stream(pg))
    return grad if Q is None else (grad, grad_src)


def check_csr_edge_frames_backward_shapes(rot, trans, row_ptr, col, in_ptr, in_edge, frame_mask=None, src_rot=None,
                                          src_trans=None, src_mask=None, grad_pos=None, grad_rot=None) -> Tuple[int, int, int, int]:
    """Shape rules of ``csr_edge_frames_backward`` (no launch): those of ``csr_edge_frames``, the incoming list of
    ``csr_incoming_edges``, and ``grad_pos`` (E,3) and ``grad_rot`` (E,3,3) floating-point, one of them given; ValueError;
    returns (B, M, Q, E)."""
    B, M, Q, E = check_csr_edge_frames_shapes(rot, trans, row_ptr, col, frame_mask, src_rot, src_trans, src_mask)
    if grad_pos is None and grad_rot is None:
        raise ValueError("nothing to compute: grad_pos and grad_rot are both None")
    _check_optional(grad_pos, (E, 3), "grad_pos", "the edges", floating=True)
    _check_optional(grad_rot, (E, 3, 3), "grad_rot", "the edges", floating=True)
    _check_incoming(in_ptr, in_edge, B, M)
    _same_device(rot, in_ptr=in_ptr, in_edge=in_edge, grad_pos=grad_pos, grad_rot=grad_rot)
    return B, M, Q, E


def csr_edge_frames_backward(rot: torch.Tensor, trans: torch.Tensor, row_ptr: torch.Tensor, col: torch.Tensor,
                             in_ptr: torch.Tensor, in_edge: torch.Tensor, frame_mask: Optional[torch.Tensor] = None, *,
                             src_rot: Optional[torch.Tensor] = None, src_trans: Optional[torch.Tensor] = None,
                             src_mask: Optional[torch.Tensor] = None, grad_pos: Optional[torch.Tensor] = None,
                             grad_rot: Optional[torch.Tensor] = None):
    """K54.  The gradient of ``csr_edge_frames`` (and of ``edge_frames``) with respect to the frames, given ``grad_pos`` (E,3)
    and / or ``grad_rot`` (E,3,3): ``(d_rot (B,M,3,3), d_trans (B,M,3))`` fp32 and, where the sources' frames are given, ``(d_rot,
    d_trans, d_src_rot (B,Q,3,3), d_src_trans (B,Q,3))``.  ``rot`` counts as nine free numbers per frame, which is what
    ``frames_backward`` takes.  One kernel walks a frame's outgoing edge positions, ascending, then its incoming ones
    (``csr_incoming_edges``), ascending, sums their terms in double from +0 and rounds once: defined bit for bit, no
    atomics.  Exactly 0 at the padding and where either frame is outside its mask; nothing is read there.  No host read;
    every element is written (include/protstruc_edgegrad.h)."""
    B, M, Q, E = check_csr_edge_frames_backward_shapes(rot, trans, row_ptr, col, in_ptr, in_edge, frame_mask, src_rot, src_trans,
                                                       src_mask, grad_pos, grad_rot)
    r, t, fm = _f32c(rot, "rot"), _f32c(trans, "trans"), _u8c(frame_mask, "frame_mask")
    sr, st, sm = _f32c_opt(src_rot, "src_rot"), _f32c_opt(src_trans, "src_trans"), _u8c(src_mask, "src_mask")
    gp, gr = _f32c_opt(grad_pos, "grad_pos"), _f32c_opt(grad_rot, "grad_rot")
    rp, cl, ip, ie = _row_ptr64(row_ptr), _col32(col, M), in_ptr.contiguous(), in_edge.contiguous()
    bipartite = sr is not None
    with _on(r.device):
        edges = bool(B and E and M and Q)   # otherwise nothing is an edge, and an empty tensor has no device pointer
        shapes = [(B, M, 3, 3), (B, M, 3)] + ([(B, Q, 3, 3), (B, Q, 3)] if bipartite else [])
        out = tuple((torch.empty if edges else torch.zeros)(shape, dtype=torch.float32, device=r.device) for shape in shapes)
        if edges:   # the kernel writes every element
            _launch_edgegrad("ps_csr_edge_frames_backward_f32", _ptr(r), _ptr(t), _ptr(fm), _ptr(sr), _ptr(st), _ptr(sm), _ptr(rp),
                             _ptr(cl), E, _ptr(ip), _ptr(ie), ie.shape[0], _ptr(gp), _ptr(gr), *(_ptr(o) for o in out),
                             *(() if bipartite else (None, None)), B, M, Q, _stream(r))
    return out


# ---- message passing on graphs (K55 - K59, include/protstruc_aggregate.h) ------------------------------------------------------
AGGREGATE_MAX_HEADS = 64  # PS_AGGREGATE_MAX_HEADS of include/protstruc_aggregate.h
AGGREGATE_MAX_ROW = 4096  # PS_AGGREGATE_MAX_ROW: H * D, the floats of one row
AGGREGATE_MODES = ("sum", "mean", "max", "min")   # by position, the modes PS_AGGREGATE_SUM .. PS_AGGREGATE_MIN


def _launch_aggregate(name: str, *args) -> None:
    """Call entry point ``name`` of libprotstruc_aggregate.so; HipLibraryError if it does not return hipSuccess."""
    rc = getattr(_aggregate.load(), name)(*args)
    if rc:
        _aggregate.check(rc, name)


def _check_rows(t, name: str, E: Optional[int] = None) -> Tuple[int, int, int]:
    """(rows, H, D) of per-edge or per-node data ``t`` (rows, H, D), floating-point, within the limits; ValueError otherwise"""
    shape = tuple(t.shape)
    if len(shape) != 3 or (E is not None and shape[0] != E):
        raise ValueError(f"{name} must have shape ({'rows' if E is None else E}, heads, floats), got {shape}")
    if not t.dtype.is_floating_point:
        raise ValueError(f"{name} must be a floating-point tensor, got {t.dtype}")
    _check_count(shape[1], 1, AGGREGATE_MAX_HEADS, f"heads in {name}")
    if shape[2] < 1 or shape[1] * shape[2] > AGGREGATE_MAX_ROW:
        raise ValueError(f"a row of {name} holds 1 .. {AGGREGATE_MAX_ROW} floats, got {shape[1]} x {shape[2]}")
    return shape


def _check_grouping(ptr, perm, row_ptr, col, B, Q, M, E: int) -> int:
    """S of a grouping over ``E`` edge positions (include/protstruc_aggregate.h): ``ptr`` (S+1,) int64 with ``perm`` None
    (the source grouping, S = B*Q) or ``perm`` (n,) int64 (the target grouping, S = B*M); ``col`` (E,) integers with
    ``row_ptr`` (B*Q+1,), or neither; ValueError otherwise."""
    _check_sizes(B=B, Q=Q, M=M)
    B, Q, M = int(B), int(Q), int(M)
    _check_batch(B)
    _check_count(Q, 0, 2 ** 24, "queries per structure")
    _check_count(M, 0, 2 ** 24, "points per structure")
    S = B * (Q if perm is None else M)
    if tuple(ptr.shape) != (S + 1,) or ptr.dtype != torch.int64:
        raise ValueError(f"ptr must be an int64 tensor of shape ({S + 1},), the {S} segments and one, got {ptr.dtype} "
                         f"{tuple(ptr.shape)}")
    if perm is not None and (perm.ndim != 1 or perm.dtype != torch.int64):
        raise ValueError(f"perm must be an int64 tensor of shape (members,), got {perm.dtype} {tuple(perm.shape)}")
    if (col is None) != (row_ptr is None):
        raise ValueError("row_ptr and col come together: the edge list the members are checked against")
    if col is not None and _check_csr_graph(row_ptr, col, B, Q, f"{B} structures") != E:
        raise ValueError(f"col must have shape ({E},), one entry per edge position, got {tuple(col.shape)}")
    _same_device(ptr, perm=perm, row_ptr=row_ptr, col=col)
    return S


def _grouping_args(ptr, perm, row_ptr, col, M: int):
    """the grouping's tensors as the kernels take them, and their six arguments (ptr, perm, n_perm, row_ptr, col)"""
    keep = (ptr.contiguous(), None if perm is None else perm.contiguous(), None if row_ptr is None else _row_ptr64(row_ptr),
            None if col is None else _col32(col, M))
    pm = keep[1] if keep[1] is not None and keep[1].shape[0] else None   # an empty tensor has no device pointer
    return keep, (_ptr(keep[0]), _ptr(pm), 0 if pm is None else pm.shape[0], _ptr(keep[2]), _ptr(keep[3]))


def check_segment_reduce_shapes(values, ptr, perm=None, weight=None, row_ptr=None, col=None, B=0, Q=0, M=0, reduce="sum",
                                return_arg=False) -> Tuple[int, int, int, int]:
    """Shape rules of ``segment_reduce`` (no launch): ValueError; returns (E, H, D, S)."""
    E, H, D = _check_rows(values, "values")
    if reduce not in AGGREGATE_MODES:
        raise ValueError(f"reduce must be one of {', '.join(AGGREGATE_MODES)}, got {reduce!r}")
    if reduce in ("max", "min") and weight is not None:
        raise ValueError(f"reduce={reduce!r} takes no weight")
    if return_arg and reduce in ("sum", "mean"):
        raise ValueError(f"reduce={reduce!r} has no arg: return_arg goes with max and min")
    _check_optional(weight, (E, H), "weight", "the edges and heads of values", floating=True)
    S = _check_grouping(ptr, perm, row_ptr, col, B, Q, M, E)
    _same_device(values, ptr=ptr, weight=weight)
    return E, H, D, S


def segment_reduce(values: torch.Tensor, ptr: torch.Tensor, perm: Optional[torch.Tensor] = None, *, B: int, Q: int, M: int,
                   reduce: str = "sum", weight: Optional[torch.Tensor] = None, row_ptr: Optional[torch.Tensor] = None,
                   col: Optional[torch.Tensor] = None, return_arg: bool = False):
    """K55.  The sum, mean, max or min of the per-edge rows ``values`` (E,H,D) over every segment of a grouping: ``out``
    (S,H,D) fp32 or, with ``return_arg`` (max, min), ``(out, arg (S,H,D) int64)``, the winning edge positions.  The source
    grouping is ``ptr = row_ptr`` with ``perm`` None (S = B*Q); the target grouping ``ptr, perm = csr_incoming_edges(...)``
    (S = B*M).  With ``row_ptr`` and ``col`` the members at the padding are skipped and nothing is read there.  Sums are in
    double from +0, members ascending, each term the exact product with ``weight`` (E,H), rounded once: defined bit for
    bit; ties of max / min go to the lower position; an empty segment gives +0 and -1.  No atomics, no host read, every
    element written (include/protstruc_aggregate.h)."""
    E, H, D, S = check_segment_reduce_shapes(values, ptr, perm, weight, row_ptr, col, B, Q, M, reduce, return_arg)
    v, wt = _f32c(values, "values"), _f32c_opt(weight, "weight")
    keep, lists = _grouping_args(ptr, perm, row_ptr, col, int(M))
    _require_device(keep[0], "ptr")
    with _on(v.device):
        if not (S and E):   # nothing to launch (an empty tensor has no device pointer): every segment is empty
            out = torch.zeros(S, H, D, dtype=torch.float32, device=v.device)
            return (out, torch.full((S, H, D), -1, dtype=torch.int64, device=v.device)) if return_arg else out
        out = torch.empty(S, H, D, dtype=torch.float32, device=v.device)   # every element is written
        arg = torch.empty(S, H, D, dtype=torch.int64, device=v.device) if return_arg else None
        _launch_aggregate("ps_segment_reduce_f32", _ptr(v), _ptr(wt), *lists, E, AGGREGATE_MODES.index(reduce), _ptr(out),
                          _ptr(arg), int(B), int(Q), int(M), H, D, _stream(v))
    return (out, arg) if return_arg else out


def _check_index(index, E: Optional[int] = None) -> int:
    if index.ndim != 1 or index.dtype != torch.int64 or (E is not None and index.shape[0] != E):
        raise ValueError(f"index must be an int64 tensor of shape ({'edges' if E is None else E},), got {index.dtype} "
                         f"{tuple(index.shape)}")
    return index.shape[0]


def check_segment_gather_shapes(node, index, weight=None) -> Tuple[int, int, int, int]:
    """Shape rules of ``segment_gather`` (no launch): ValueError; returns (E, S, H, D)."""
    S, H, D = _check_rows(node, "node")
    E = _check_index(index)
    _check_optional(weight, (E, H), "weight", "the edges of index and the heads of node", floating=True)
    _same_device(node, index=index, weight=weight)
    return E, S, H, D


def segment_gather(node: torch.Tensor, index: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K56.  The node rows ``node`` (S,H,D) on every edge, the adjoint of the segment sum: ``out`` (E,H,D) fp32,
    ``out[e] = weight[e] * node[index[e]]`` per head (the exact product rounded once), or a copy without ``weight`` (E,H).
    ``index`` (E,) int64 is a flat node index; outside [0, S) -- the caller's mark for the padding -- the row is exactly
    +0 and nothing is read, the weight included.  No host read; every element written (include/protstruc_aggregate.h)."""
    E, S, H, D = check_segment_gather_shapes(node, index, weight)
    nd, wt, ix = _f32c(node, "node"), _f32c_opt(weight, "weight"), index.contiguous()
    _require_device(ix, "index")
    with _on(nd.device):
        if not (E and S):
            return torch.zeros(E, H, D, dtype=torch.float32, device=nd.device)
        out = torch.empty(E, H, D, dtype=torch.float32, device=nd.device)
        _launch_aggregate("ps_segment_gather_f32", _ptr(nd), _ptr(wt), _ptr(ix), E, S, H, D, _ptr(out), _stream(nd))
    return out


def check_edge_dot_shapes(node, values, index) -> Tuple[int, int, int, int]:
    """Shape rules of ``edge_dot`` (no launch): ValueError; returns (E, S, H, D)."""
    S, H, D = _check_rows(node, "node")
    E = _check_index(index)
    if tuple(values.shape) != (E, H, D) or not values.dtype.is_floating_point:
        raise ValueError(f"values must be a floating-point tensor of shape {(E, H, D)} to match index and node, got "
                         f"{values.dtype} {tuple(values.shape)}")
    _same_device(node, index=index, values=values)
    return E, S, H, D


def edge_dot(node: torch.Tensor, values: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """K57.  ``out[e, h] = sum_d node[index[e], h, d] * values[e, h, d]``, (E,H) fp32: the gradient of a weight.  Exact
    products, summed in double in the fixed order of the header (fours ascending, then a tree) and rounded once, whatever
    the alignment; exactly +0 where ``index`` is outside [0, S), and nothing is read there (include/protstruc_aggregate.h)."""
    E, S, H, D = check_edge_dot_shapes(node, values, index)
    nd, v, ix = _f32c(node, "node"), _f32c(values, "values"), index.contiguous()
    _require_device(ix, "index")
    with _on(nd.device):
        if not (E and S):
            return torch.zeros(E, H, dtype=torch.float32, device=nd.device)
        out = torch.empty(E, H, dtype=torch.float32, device=nd.device)
        _launch_aggregate("ps_edge_dot_f32", _ptr(nd), _ptr(v), _ptr(ix), E, S, H, D, _ptr(out), _stream(nd))
    return out


def _check_heads(t, name: str) -> Tuple[int, int]:
    if t.ndim != 2 or not t.dtype.is_floating_point:
        raise ValueError(f"{name} must be a floating-point tensor of shape (edges, heads), got {t.dtype} {tuple(t.shape)}")
    _check_count(t.shape[1], 1, AGGREGATE_MAX_HEADS, f"heads in {name}")
    return tuple(t.shape)


def check_segment_softmax_shapes(logits, ptr, perm=None, row_ptr=None, col=None, B=0, Q=0, M=0) -> Tuple[int, int, int]:
    """Shape rules of ``segment_softmax`` (no launch): ValueError; returns (E, H, S)."""
    E, H = _check_heads(logits, "logits")
    S = _check_grouping(ptr, perm, row_ptr, col, B, Q, M, E)
    _same_device(logits, ptr=ptr)
    return E, H, S


def segment_softmax(logits: torch.Tensor, ptr: torch.Tensor, perm: Optional[torch.Tensor] = None, *, B: int, Q: int, M: int,
                    row_ptr: Optional[torch.Tensor] = None, col: Optional[torch.Tensor] = None, return_lse: bool = False):
    """K58.  The softmax of ``logits`` (E,H) over every segment of a grouping (see ``segment_reduce``), per head: ``w`` (E,H)
    fp32 or, with ``return_lse``, ``(w, lse (S,H))``.  The maximum is subtracted, the exponentials are evaluated and summed
    in double, members ascending, and each weight is rounded once.  A segment of one member gives exactly 1; a logit of
    -inf gives +0; an empty segment, or one whose maximum is -inf, gives weights +0 and ``lse`` -inf; ``w`` is +0 at the
    padding and nothing is read there.  No atomics, no host read (include/protstruc_aggregate.h)."""
    E, H, S = check_segment_softmax_shapes(logits, ptr, perm, row_ptr, col, B, Q, M)
    x = _f32c(logits, "logits")
    keep, lists = _grouping_args(ptr, perm, row_ptr, col, int(M))
    _require_device(keep[0], "ptr")
    with _on(x.device):
        if not (S and E):
            w = torch.zeros(E, H, dtype=torch.float32, device=x.device)
            return (w, torch.full((S, H), float("-inf"), dtype=torch.float32, device=x.device)) if return_lse else w
        w = torch.empty(E, H, dtype=torch.float32, device=x.device)   # zeroed by the entry point's first launch
        lse = torch.empty(S, H, dtype=torch.float32, device=x.device) if return_lse else None
        _launch_aggregate("ps_segment_softmax_f32", _ptr(x), *lists, E, _ptr(w), _ptr(lse), int(B), int(Q), int(M), H, _stream(x))
    return (w, lse) if return_lse else w


def check_segment_softmax_backward_shapes(w, grad_w, ptr, perm=None, row_ptr=None, col=None, B=0, Q=0, M=0) -> Tuple[int, int, int]:
    """Shape rules of ``segment_softmax_backward`` (no launch): ValueError; returns (E, H, S)."""
    E, H = _check_heads(w, "w")
    if tuple(grad_w.shape) != (E, H) or not grad_w.dtype.is_floating_point:
        raise ValueError(f"grad_w must be a floating-point tensor of shape {(E, H)} to match w, got {grad_w.dtype} "
                         f"{tuple(grad_w.shape)}")
    S = _check_grouping(ptr, perm, row_ptr, col, B, Q, M, E)
    _same_device(w, grad_w=grad_w, ptr=ptr)
    return E, H, S


def segment_softmax_backward(w: torch.Tensor, grad_w: torch.Tensor, ptr: torch.Tensor, perm: Optional[torch.Tensor] = None, *,
                             B: int, Q: int, M: int, row_ptr: Optional[torch.Tensor] = None,
                             col: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K59.  The gradient of ``segment_softmax`` with respect to the logits, (E,H) fp32, given its output ``w`` and the
    incoming ``grad_w``: per segment and head ``t = sum w * g`` in double, members ascending, and ``w * (g - t)`` rounded
    once -- defined bit for bit given ``w``; +0 at the padding, where no gradient is read (include/protstruc_aggregate.h)."""
    E, H, S = check_segment_softmax_backward_shapes(w, grad_w, ptr, perm, row_ptr, col, B, Q, M)
    ww, g = _f32c(w, "w"), _f32c(grad_w, "grad_w")
    keep, lists = _grouping_args(ptr, perm, row_ptr, col, int(M))
    _require_device(keep[0], "ptr")
    with _on(ww.device):
        if not (S and E):
            return torch.zeros(E, H, dtype=torch.float32, device=ww.device)
        gx = torch.empty(E, H, dtype=torch.float32, device=ww.device)
        _launch_aggregate("ps_segment_softmax_backward_f32", _ptr(ww), _ptr(g), *lists, E, _ptr(gx), int(B), int(Q), int(M), H,
                          _stream(ww))
    return gx


CHI_MAX_TYPES = 32  # PS_CHI_MAX_TYPES of include/protstruc_hip.h: the tables travel in the kernel's arguments


def _host_i32_table(values, shape_tail, name: str) -> np.ndarray:
    """A host table of the chi kernels as a contiguous int32 array of shape (T, *shape_tail), 1 <= T <= CHI_MAX_TYPES."""
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().numpy()
    try:
        arr = np.asarray(values)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be an integer array of shape (types, {', '.join(map(str, shape_tail))})") from None
    if arr.ndim != 1 + len(shape_tail) or arr.shape[1:] != tuple(shape_tail) or arr.dtype.kind not in "iu":
        raise ValueError(f"{name} must be an integer array of shape (types, {', '.join(map(str, shape_tail))}), got "
                         f"{arr.dtype} {arr.shape}")
    if not 1 <= arr.shape[0] <= CHI_MAX_TYPES:
        raise ValueError(f"{name} must hold 1 .. {CHI_MAX_TYPES} residue types, got {arr.shape[0]}")
    return np.ascontiguousarray(arr.astype(np.int64).clip(-2, 2 ** 31 - 1).astype(np.int32))


def _chi_tables(chi_atoms, chi_last, A: int, with_last: bool):
    """The validated host tables (chi_atoms (T,4,4) int32, chi_last (T,4) int32 or None): the library's own rules."""
    if chi_atoms is None or (with_last and chi_last is None):
        raise ValueError("chi_atoms" + (" and chi_last are" if with_last else " is") + " required "
                         "(general.chi_atom_table()" + (", general.chi_last_table())" if with_last else ")"))
    atoms = _host_i32_table(chi_atoms, (4, 4), "chi_atoms")
    T = atoms.shape[0]
    none = (atoms == -1).all(-1)
    inside = ((atoms >= 0) & (atoms < A)).all(-1)
    distinct = np.array([[len(set(row.tolist())) == 4 for row in per_type] for per_type in atoms])
    if not (none | (inside & distinct)).all():
        t, k = np.argwhere(~(none | (inside & distinct)))[0]
        raise ValueError(f"chi_atoms[{t}][{k}] = {atoms[t, k].tolist()} must be all -1 or four distinct atom slots in [0, {A})")
    if not with_last:
        return atoms, None
    last = _host_i32_table(chi_last, (4,), "chi_last")
    if last.shape[0] != T:
        raise ValueError(f"chi_last must hold the {T} residue types of chi_atoms, got {last.shape[0]}")
    d = atoms[:, :, 3]
    ok = (last == -1) | (~none & (last >= d) & (last < A)
                         & ~((atoms[:, :, :3] >= d[..., None]) & (atoms[:, :, :3] <= last[..., None])).any(-1))
    if not ok.all():
        t, k = np.argwhere(~ok)[0]
        raise ValueError(f"chi_last[{t}][{k}] = {last[t, k]} must be -1, or in [d, {A}) with none of a, b, c of "
                         f"chi_atoms[{t}][{k}] = {atoms[t, k].tolist()} inside [d, last]")
    return atoms, last


def _check_residue_type(residue_type, B: int, N: int, like: str) -> None:
    if tuple(residue_type.shape) != (B, N):
        raise ValueError(f"residue_type must have shape {(B, N)} to match {like}, got {tuple(residue_type.shape)}")
    if not _is_integer_tensor(residue_type):
        raise ValueError(f"residue_type must be an integer tensor, got {residue_type.dtype}")


def _chi_dims(xyz) -> Tuple[int, int, int]:
    B, N, A = _xyz_dims(xyz)
    _check_count(B * N, 0, 2 ** 31, "residues per call")
    _check_count(A, 1, 64, "atom slots per residue")
    return B, N, A


def _type32(residue_type: torch.Tensor, T: int) -> torch.Tensor:
    """``residue_type`` as contiguous int32 for the chi kernels, to which every value outside [0, T) is padding: wider
    integers are clamped to [-1, T] first, so that none wraps into the range."""
    _require_device(residue_type, "residue_type")
    if residue_type.dtype != torch.int32:
        residue_type = residue_type.clamp(-1, T).to(torch.int32)
    return residue_type.contiguous()


def _ints(table: Optional[np.ndarray]):
    return None if table is None else (ctypes.c_int * table.size)(*table.ravel().tolist())


def check_chi_shapes(xyz, residue_type, atom_mask=None, chi_atoms=None, grad_chi=None, want_chi=True, want_mask=True) -> None:
    """Shape rules of ``chi`` / ``chi_backward``, on shapes, dtypes, devices and the host table only (no launch):
    ValueError.  ``xyz`` (B,N,A,3) floating point with ``B * N <= 2^31`` and ``1 <= A <= 64``; ``residue_type`` (B,N)
    integers; ``atom_mask`` (B,N,A); ``chi_atoms`` (T,4,4) integers, ``1 <= T <= CHI_MAX_TYPES``, every angle all -1 or
    four distinct slots in [0, A); ``grad_chi`` (B,N,4) floating point; one of the two outputs wanted."""
    _checked_chi(xyz, residue_type, atom_mask, chi_atoms, grad_chi, want_chi, want_mask)


def _checked_chi(xyz, residue_type, atom_mask, chi_atoms, grad_chi, want_chi=True, want_mask=True) -> np.ndarray:
    """``check_chi_shapes``; returns the validated host table."""
    B, N, A = _chi_dims(xyz)
    shape = (B, N, A, 3)
    _check_residue_type(residue_type, B, N, f"xyz {shape}")
    _check_optional(atom_mask, (B, N, A), "atom_mask", "xyz", shape)
    atoms, _ = _chi_tables(chi_atoms, None, A, False)
    _check_optional(grad_chi, (B, N, 4), "grad_chi", "xyz", shape, floating=True)
    if not (want_chi or want_mask):
        raise ValueError("nothing to compute: want_chi and want_mask are both False")
    _same_device(xyz, residue_type=residue_type, atom_mask=atom_mask, grad_chi=grad_chi)
    return atoms


def chi(xyz: torch.Tensor, residue_type: torch.Tensor, atom_mask: Optional[torch.Tensor] = None, *, chi_atoms,
        want_chi: bool = True, want_mask: bool = True):
    """K27.  The side-chain torsions of every residue: ``(chi (B,N,4) fp32, chi_mask (B,N,4) bool)``, None for an output
    not wanted.  ``chi_atoms`` (T,4,4) is the host table of the four atom slots a, b, c, d of angle k of residue type t
    (``general.chi_atom_table()``), ``residue_type`` (B,N) the row of each residue -- a value outside [0, T) is padding
    --, ``atom_mask`` (B,N,A; None = all).  An angle is defined where the table has it and its four atoms are in the mask:
    ``chi = atan2((m . b1) / |b1|, n1 . n2)`` with ``b0 = a - b, b1 = c - b, b2 = d - c, n1 = b0 x b1, n2 = b2 x b1, m = n1 x
    n2`` in double on the float32 coordinates, rounded once (``geometry.dihedral``'s sign); exact 0 and mask False
    elsewhere, whatever NaN sits under the mask (include/protstruc_hip.h)."""
    atoms = _checked_chi(xyz, residue_type, atom_mask, chi_atoms, None, want_chi, want_mask)
    x, am = _f32c(xyz, "xyz"), _u8c(atom_mask, "atom_mask")
    B, N, A = x.shape[:3]
    rt = _type32(residue_type, atoms.shape[0])
    with _on(x.device):
        out = torch.empty(B, N, 4, dtype=torch.float32, device=x.device) if want_chi else None
        mask = torch.empty(B, N, 4, dtype=torch.bool, device=x.device) if want_mask else None
        if B and N:
            _launch("ps_chi_f32", _ptr(x), _ptr(am), _ptr(rt), _ints(atoms), atoms.shape[0], _ptr(out), _ptr(mask), B, N, A,
                    _stream(x))
    return out, mask


def chi_backward(xyz: torch.Tensor, residue_type: torch.Tensor, grad_chi: torch.Tensor,
                 atom_mask: Optional[torch.Tensor] = None, *, chi_atoms) -> torch.Tensor:
    """K28.  Vector-Jacobian product of ``chi`` in one launch: ``grad_xyz`` (B,N,A,3) fp32 from the upstream ``grad_chi``
    (B,N,4).  The lane that owns a residue sums the contributions of its angles per atom in double, in the order k =
    0..3, and writes the whole row: exact zeros in the slots no defined angle reads; ``grad_chi`` is not read at an
    undefined angle; no atomics, deterministic (include/protstruc_hip.h)."""
    atoms = _checked_chi(xyz, residue_type, atom_mask, chi_atoms, grad_chi)
    x, am, g = _f32c(xyz, "xyz"), _u8c(atom_mask, "atom_mask"), _f32c(grad_chi, "grad_chi")
    B, N, A = x.shape[:3]
    rt = _type32(residue_type, atoms.shape[0])
    with _on(x.device):
        out = torch.empty(B, N, A, 3, dtype=torch.float32, device=x.device)
        if B and N:
            _launch("ps_chi_backward_f32", _ptr(x), _ptr(am), _ptr(rt), _ints(atoms), atoms.shape[0], _ptr(g), _ptr(out),
                    B, N, A, _stream(x))
    return out


def check_chi_set_shapes(xyz, chi, residue_type, atom_mask=None, chi_select=None, chi_atoms=None, chi_last=None,
                         grad_out=None) -> None:
    """Shape rules of ``chi_set`` / ``chi_set_backward``, on shapes, dtypes, devices and the host tables only (no
    launch): ValueError.  As ``check_chi_shapes``, with ``chi`` (B,N,4) floating point (None for the backward pass),
    ``chi_select`` (B,N,4), ``chi_last`` (T,4) integers -- -1, or in [d, A) with none of a, b, c inside [d, last] -- and
    ``grad_out`` of the shape of ``xyz``."""
    _checked_chi_set(xyz, chi, residue_type, atom_mask, chi_select, chi_atoms, chi_last, grad_out)


def _checked_chi_set(xyz, chi, residue_type, atom_mask, chi_select, chi_atoms, chi_last, grad_out=None):
    """``check_chi_set_shapes``; returns the validated host tables."""
    B, N, A = _chi_dims(xyz)
    shape = (B, N, A, 3)
    _check_optional(chi, (B, N, 4), "chi", "xyz", shape, floating=True)
    _check_residue_type(residue_type, B, N, f"xyz {shape}")
    _check_optional(atom_mask, (B, N, A), "atom_mask", "xyz", shape)
    _check_optional(chi_select, (B, N, 4), "chi_select", "xyz", shape)
    tables = _chi_tables(chi_atoms, chi_last, A, True)
    _check_optional(grad_out, shape, "grad_out", "xyz", shape, floating=True)
    _same_device(xyz, chi=chi, residue_type=residue_type, atom_mask=atom_mask, chi_select=chi_select, grad_out=grad_out)
    return tables


def chi_set(xyz: torch.Tensor, chi: torch.Tensor, residue_type: torch.Tensor, atom_mask: Optional[torch.Tensor] = None,
            chi_select: Optional[torch.Tensor] = None, *, chi_atoms, chi_last, relative: bool = False) -> torch.Tensor:
    """K29.  The coordinates with the side chains turned to the angles ``chi`` (B,N,4) -- by them if ``relative`` --: a
    new (B,N,A,3) fp32 tensor.  For k = 0..3 in this order, where angle k is defined (``chi``), ``chi_last[t][k] >= 0``
    (``general.chi_last_table()``: the last slot the angle moves; -1 = never turned, as proline's) and ``chi_select``
    (B,N,4; None = all) is non-zero, the present slots [d, last] of the residue's current coordinates are rotated about
    b -> c by ``chi[k] - measured`` (``chi[k]`` if relative), in double, rounded once at the store.  Every other float is
    the input's bit pattern, NaN of missing atoms and padding included; ``chi`` is not read where it is not used
    (include/protstruc_hip.h)."""
    atoms, last = _checked_chi_set(xyz, chi, residue_type, atom_mask, chi_select, chi_atoms, chi_last)
    x, c, am, sel = _f32c(xyz, "xyz"), _f32c(chi, "chi"), _u8c(atom_mask, "atom_mask"), _u8c(chi_select, "chi_select")
    B, N, A = x.shape[:3]
    rt = _type32(residue_type, atoms.shape[0])
    with _on(x.device):
        out = torch.empty(B, N, A, 3, dtype=torch.float32, device=x.device)
        if B and N:
            _launch("ps_chi_set_f32", _ptr(x), _ptr(am), _ptr(rt), _ints(atoms), _ints(last), atoms.shape[0], _ptr(c),
                    _ptr(sel), int(bool(relative)), _ptr(out), B, N, A, _stream(x))
    return out


def chi_set_backward(out: torch.Tensor, grad_out: torch.Tensor, residue_type: torch.Tensor,
                     atom_mask: Optional[torch.Tensor] = None, chi_select: Optional[torch.Tensor] = None, *, chi_atoms,
                     chi_last) -> torch.Tensor:
    """K30.  Vector-Jacobian product of ``chi_set`` towards the angles: ``grad_chi`` (B,N,4) fp32 from the upstream
    ``grad_out`` (B,N,A,3) and the coordinates ``out`` that ``chi_set`` returned, with its masks and tables:
    ``grad_chi[k] = sum_s (u_k x (p_s - c_k)) . g_s`` over the present slots angle k turned, in double; exact 0 at an
    angle that was not turned.  The whole derivative in both modes; there is no gradient towards ``xyz``."""
    atoms, last = _checked_chi_set(out, None, residue_type, atom_mask, chi_select, chi_atoms, chi_last, grad_out)
    x, g, am, sel = _f32c(out, "out"), _f32c(grad_out, "grad_out"), _u8c(atom_mask, "atom_mask"), _u8c(chi_select, "chi_select")
    B, N, A = x.shape[:3]
    rt = _type32(residue_type, atoms.shape[0])
    with _on(x.device):
        grad = torch.empty(B, N, 4, dtype=torch.float32, device=x.device)
        if B and N:
            _launch("ps_chi_set_backward_f32", _ptr(x), _ptr(am), _ptr(rt), _ints(atoms), _ints(last), atoms.shape[0],
                    _ptr(sel), _ptr(g), _ptr(grad), B, N, A, _stream(x))
    return grad


def diffuse_(xyz: torch.Tensor, beta: torch.Tensor, rng_state: Optional[torch.Tensor] = None,
             noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K5, in place on a contiguous fp32 ``xyz``.  ``rng_state``: int64 device tensor of RNG_STATE_WORDS
    words, [0] = seed, [1] = draw offset, the rest zero."""
    _require_f32c(xyz, "xyz", "diffuse_ needs a contiguous float32 xyz (it is updated in place)")
    B = xyz.shape[0]
    nps = xyz[0].numel() if B else 0
    beta, noise = _diffusion_operands(xyz, beta, rng_state, noise)
    with _on(xyz.device):
        if not (xyz.numel() == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_diffuse_f32", _ptr(xyz), _ptr(beta), B, nps, _ptr(rng_state), _ptr(noise), _stream(xyz))
    return xyz


def diffuse_frames_(xyz: torch.Tensor, beta: torch.Tensor, a1: int, a2: int, a3: int, t_atom: int = 1,
                    rng_state: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                    out_rot: Optional[torch.Tensor] = None, out_trans: Optional[torch.Tensor] = None):
    """Fused K5 + K4: diffuse ``xyz`` in place and return the frames of the new coordinates."""
    _require_f32c(xyz, "xyz", "diffuse_frames_ needs a contiguous float32 xyz (it is updated in place)")
    B, N, A = xyz.shape[:3]
    beta, noise = _diffusion_operands(xyz, beta, rng_state, noise)
    _check_atom_slots(A, a1, a2, a3, t_atom)
    dev = xyz.device
    _check_out(out_rot, (B, N, 3, 3), "out_rot", dev)
    _check_out(out_trans, (B, N, 3), "out_trans", dev)
    with _on(dev):
        rot = out_rot if out_rot is not None else torch.empty(B, N, 3, 3, dtype=torch.float32, device=dev)
        trans = out_trans if out_trans is not None else torch.empty(B, N, 3, dtype=torch.float32, device=dev)
        if not (xyz.numel() == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_diffuse_frames_f32", _ptr(xyz), _ptr(beta), B, N, A, _ptr(rng_state), _ptr(noise), _ptr(rot),
                    _ptr(trans), int(a1), int(a2), int(a3), int(t_atom), _stream(xyz))
    return rot, trans


def diffusion_trajectory_(xyz: torch.Tensor, betas: torch.Tensor, a1: int, a2: int, a3: int, t_atom: int,
                          rng_state: torch.Tensor, want_rot: bool = True, want_trans: bool = True,
                          want_xyz: bool = False, *, out_rot: Optional[torch.Tensor] = None,
                          out_trans: Optional[torch.Tensor] = None, out_xyz: Optional[torch.Tensor] = None):
    """K55: T diffusion steps in one launch, coordinates resident in LDS.  ``betas``: (T, B).
    Returns (rot (T,B,N,3,3) | None, trans (T,B,N,3) | None, xyz_traj (T,B,N,A,3) | None); ``xyz`` ends as step T.
    ``out_rot`` / ``out_trans`` / ``out_xyz`` supply caller-owned output buffers (and imply the matching ``want_``)."""
    _require_f32c(xyz, "xyz", "diffusion_trajectory_ needs a contiguous float32 xyz (it is updated in place)")
    B, N, A = xyz.shape[:3]
    betas = _f32c(betas, "betas")
    if betas.ndim != 2 or betas.shape[1] != B:
        raise ValueError(f"betas must have shape (T, {B}), got {tuple(betas.shape)}")
    T = betas.shape[0]
    if rng_state is None:
        raise ValueError(f"rng_state must be an int64 tensor of {RNG_STATE_WORDS} words")
    _check_rng_state(rng_state, xyz.device)
    _check_atom_slots(A, a1, a2, a3, t_atom)
    dev = xyz.device
    _same_device(xyz, betas=betas)
    _check_out(out_rot, (T, B, N, 3, 3), "out_rot", dev)
    _check_out(out_trans, (T, B, N, 3), "out_trans", dev)
    _check_out(out_xyz, (T, B, N, A, 3), "out_xyz", dev)
    with _on(dev):
        rot = out_rot if out_rot is not None else (
            torch.empty(T, B, N, 3, 3, dtype=torch.float32, device=dev) if want_rot else None)
        trans = out_trans if out_trans is not None else (
            torch.empty(T, B, N, 3, dtype=torch.float32, device=dev) if want_trans else None)
        traj = out_xyz if out_xyz is not None else (
            torch.empty(T, B, N, A, 3, dtype=torch.float32, device=dev) if want_xyz else None)
        if not (xyz.numel() == 0 or T == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_diffusion_trajectory_f32", _ptr(xyz), _ptr(betas), T, B, N, A, _ptr(rng_state), _ptr(rot),
                    _ptr(trans), _ptr(traj), int(a1), int(a2), int(a3), int(t_atom), _stream(xyz))
    return rot, trans, traj


def standardize_(xyz: torch.Tensor, atom_mask: Optional[torch.Tensor]):
    """K6, in place.  Returns (mu (B,3), std (B,3))."""
    _require_f32c(xyz, "xyz", "standardize_ needs a contiguous float32 xyz (it is updated in place)")
    B, N, A = xyz.shape[:3]
    m = _u8c(atom_mask, "atom_mask")
    dev = xyz.device
    with _on(dev):
        # a structure without atoms has 0 / 0 statistics in the reference: NaN, not uninitialised memory
        alloc = torch.empty if N * A > 0 else (lambda *a, **k: torch.full(a, float("nan"), **k))
        mu = alloc(B, 3, dtype=torch.float32, device=dev)
        std = alloc(B, 3, dtype=torch.float32, device=dev)
        if not (xyz.numel() == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_standardize_f32", _ptr(xyz), _ptr(m), _ptr(mu), _ptr(std), B, N, A, _stream(xyz))
    return mu, std


def affine_(xyz: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """xyz[b] <- xyz[b] * scale[b] + shift[b] per axis, in place (unstandardize)."""
    _require_f32c(xyz, "xyz", "affine_ needs a contiguous float32 xyz (it is updated in place)")
    B = xyz.shape[0]
    n_atoms = xyz[0].numel() // 3 if B else 0
    scale = _f32c(scale, "scale")
    shift = _f32c(shift, "shift")
    with _on(xyz.device):
        if not (xyz.numel() == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_affine_f32", _ptr(xyz), _ptr(scale), _ptr(shift), B, n_atoms, _stream(xyz))
    return xyz


def check_rigid_shapes(xyz, R=None, t=None) -> Tuple[int, int]:
    """Shape rules of ``rigid``, on shapes only (no launch): ValueError.  Returns the kernel's (r_mode, t_mode)."""
    B, N, A = _xyz_dims(xyz, floating=False)
    r_mode = t_mode = 0
    if R is not None:
        r_mode = {2: 1, 3: 2, 4: 3}.get(R.ndim, -1)
        ok = tuple(R.shape[-2:]) == (3, 3) and (r_mode == 1 or (R.shape[0] == B and (r_mode == 2 or R.shape[1] == N)))
        if r_mode < 0 or not ok:
            raise ValueError(f"rotation must be (3,3), ({B},3,3) or ({B},{N},3,3), got {tuple(R.shape)}")
    if t is not None:
        t_shape = tuple(t.shape)
        if t_shape == (3,) or t_shape == (1, 3):
            t_mode = 1
        elif t_shape == (B, 3) or t_shape == (B, 1, 3):
            t_mode = 2
        elif t_shape == (B, N, 3):
            t_mode = 3
        elif t_shape == (B, N, A, 3):
            t_mode = 4
        else:
            raise ValueError(f"translation shape {t_shape} does not broadcast against xyz {(B, N, A, 3)}")
    return r_mode, t_mode


def rigid(xyz: torch.Tensor, R: Optional[torch.Tensor] = None, t: Optional[torch.Tensor] = None, *,
          transpose: bool = False, inplace: bool = False) -> torch.Tensor:
    """x' = R x + t (or R^T x + t).  R: (3,3) | (B,3,3) | (B,N,3,3);  t: (3,) | (1,3) | (B,3) | (B,1,3) | (B,N,3) | (B,N,A,3)."""
    r_mode, t_mode = check_rigid_shapes(xyz, R, t)
    _require_f32c(xyz, "xyz", "rigid needs a contiguous float32 xyz")
    B, N, A = xyz.shape[:3]
    if R is not None:
        R = _f32c(R, "rotation")
    if t is not None:
        t = _f32c(t, "translation")
    with _on(xyz.device):
        out = xyz if inplace else torch.empty_like(xyz)
        if not (xyz.numel() == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_rigid_f32", _ptr(xyz), _ptr(out), _ptr(R), r_mode, int(transpose), _ptr(t), t_mode, B, N, A,
                    _stream(xyz))
    return out


def center_of_mass(xyz: torch.Tensor, atom: int = 1) -> torch.Tensor:
    """(B,3) nanmean over residues of one atom slot, per component (a residue with a NaN y still counts for x and z);
    NaN where no residue has the component.  Accumulated in double and rounded once."""
    B, N, A = _xyz_dims(xyz, floating=False)
    if A:
        _check_atom_slots(A, atom)
    xyz = _f32c(xyz, "xyz")
    with _on(xyz.device):
        # no residues: the reference's nanmean over nothing is NaN
        com = (torch.empty if xyz.numel() else (lambda *a, **k: torch.full(a, float("nan"), **k)))(
            B, 3, dtype=torch.float32, device=xyz.device)
        if not (xyz.numel() == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_center_of_mass_f32", _ptr(xyz), _ptr(com), B, N, A, int(atom), _stream(xyz))
    return com


def frames_to_backbone(rot: torch.Tensor, trans: torch.Tensor, ideal: torch.Tensor, n_slots: int) -> torch.Tensor:
    """(B,N,n_slots,3): rot @ ideal[a] + trans for the first len(ideal) slots, zeros after."""
    rot = _f32c(rot, "orientations")
    trans = _f32c(trans, "translations")
    B, N = rot.shape[:2]
    if rot.shape != (B, N, 3, 3) or trans.shape != (B, N, 3):
        raise ValueError("orientations must be (B,N,3,3) and translations (B,N,3)")
    ideal = _f32c(ideal.to(rot.device), "ideal")
    with _on(rot.device):
        xyz = torch.empty(B, N, n_slots, 3, dtype=torch.float32, device=rot.device)
        if not (xyz.numel() == 0):   # empty input: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_frames_to_backbone_f32", _ptr(rot), _ptr(trans), _ptr(ideal), ideal.shape[0], _ptr(xyz), B, N,
                    n_slots, _stream(rot))
    return xyz


def check_kabsch_shapes(src, dst, atom_mask) -> Tuple[int, int, bool, bool]:
    """Shape rules of ``kabsch``, on shapes only (no launch): ValueError.  ``src`` is (B, ..., 3) with n = the product of
    the middle axes atoms per structure, ``dst`` (B or 1, ..., 3) with the same n, ``atom_mask`` any shape of B n or n
    entries.  Returns (B, n, one target for all, one mask for all)."""
    for name, x in (("source", src), ("target", dst)):
        if x.ndim < 2 or x.shape[-1] != 3:
            raise ValueError(f"{name} xyz must have shape (batch, ..., 3), got {tuple(x.shape)}")
    B = src.shape[0]
    n_atoms = int(np.prod(src.shape[1:-1], dtype=np.int64))
    if int(np.prod(dst.shape[1:-1], dtype=np.int64)) != n_atoms:
        raise ValueError(f"source and target must have the same number of atoms per structure, got {tuple(src.shape)} "
                         f"and {tuple(dst.shape)}")
    if dst.shape[0] not in (1, B):
        raise ValueError(f"the target must have the batch size of the source ({B}) or 1, got {dst.shape[0]}")
    count = atom_mask.numel()
    if count not in (n_atoms, B * n_atoms):
        if n_atoms and count and count % n_atoms == 0:
            raise ValueError(f"atom_mask must have the batch size of the source ({B}) or 1, got {count // n_atoms}")
        raise ValueError(f"atom_mask must have {n_atoms} entries per structure, got {tuple(atom_mask.shape)} against "
                         f"source {tuple(src.shape)}")
    return B, n_atoms, dst.shape[0] == 1 and B > 1, count == n_atoms and B > 1


def kabsch(src: torch.Tensor, dst: torch.Tensor, atom_mask: torch.Tensor):
    """Per-structure optimal (R (B,3,3), t (B,3)) taking ``src`` (B,N,A,3) onto ``dst`` ((B|1),N,A,3) over masked atoms.

    R is always a proper rotation (R R^T = I, det R = +1), whatever the selection: a mirror-image target gets the best
    rotation, not the reflection.  Where the covariance is rank-deficient (two atoms, collinear atoms) the optimum is a
    family and R is one member of it, with the optimal RMSD.  One selected atom, or coincident selected atoms: R = I and
    t = b - a (the reference's result).  No selected atom (an empty mask, or no atoms at all): R and t are NaN, the
    reference's 0 / 0.  Masked-out atoms are never read (include/protstruc_hip.h)."""
    B, n_atoms, dst_shared, mask_shared = check_kabsch_shapes(src, dst, atom_mask)
    src = _f32c(src, "source xyz")
    dst = _f32c(dst.to(src.device), "target xyz")
    m = _u8c(atom_mask.to(src.device), "atom_mask")
    dev = src.device
    with _on(dev):
        if B == 0 or n_atoms == 0:   # nothing to launch (an empty tensor has no device pointer): no atom is selected
            return (torch.full((B, 3, 3), float("nan"), dtype=torch.float32, device=dev),
                    torch.full((B, 3), float("nan"), dtype=torch.float32, device=dev))
        R = torch.empty(B, 3, 3, dtype=torch.float32, device=dev)
        t = torch.empty(B, 3, dtype=torch.float32, device=dev)
        _launch("ps_kabsch_f32", _ptr(src), _ptr(dst), _ptr(m), _ptr(R), _ptr(t), B, n_atoms,
                int(dst_shared), int(mask_shared), _stream(src))
    return R, t


def check_min_dist_shapes(xyz_one, query, atom: int = 1) -> Tuple[int, int, int]:
    """Shape rules of ``min_dist_to_points``, on shapes only (no launch): ValueError.  ``xyz_one`` is ONE structure
    (N,A,3), ``query`` (..., 3) with at least one point -- the reference's min over no point raises as well -- and
    ``atom`` a slot of xyz_one.  Returns (N, A, query points)."""
    shape = tuple(xyz_one.shape)
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"xyz must be one structure of shape (residues, atoms, 3), got {shape}")
    if query.ndim < 1 or query.shape[-1] != 3:
        raise ValueError(f"query_xyz must have shape (..., 3), got {tuple(query.shape)}")
    if query.numel() == 0:
        raise ValueError("query_xyz holds no point: the nearest of no points is undefined")
    _check_atom_slots(shape[1], atom)
    return shape[0], shape[1], query.numel() // 3


def min_dist_to_points(xyz_one: torch.Tensor, query: torch.Tensor, atom: int = 1) -> torch.Tensor:
    """(N,) distance from atom slot ``atom`` of each residue of one structure (N,A,3) to its nearest query point.  A NaN
    query point turns every entry NaN, a NaN atom its own entry; zero query points raise ValueError."""
    N, A, n_query = check_min_dist_shapes(xyz_one, query, atom)
    xyz_one = _f32c(xyz_one, "xyz")
    query = _f32c(query.to(xyz_one.device), "query_xyz").reshape(-1, 3)
    with _on(xyz_one.device):
        out = torch.empty(N, dtype=torch.float32, device=xyz_one.device)
        if N:   # no residue: nothing to launch (an empty tensor has no device pointer)
            _launch("ps_min_dist_to_points_f32", _ptr(xyz_one), _ptr(query), _ptr(out), N, A, int(atom), n_query,
                    _stream(xyz_one))
    return out
