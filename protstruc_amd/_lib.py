"""ctypes binding of libprotstruc_hip.so (C ABI: include/protstruc_hip.h and the side headers listed in ``FAMILIES``).

There is deliberately no fallback: if the shared library is missing or a launch
fails, the caller gets an exception -- never a silent CPU / eager-PyTorch path.
"""
import contextlib
import ctypes
import os
import threading
from typing import NamedTuple

from ._headers import HipLibraryError, prototypes, struct_fields  # noqa: F401 -- HipLibraryError is this module's error too

_HERE = os.path.dirname(os.path.abspath(__file__))
# PROTSTRUC_AMD_LIB selects another build of the library: the same-process A/B of two builds (tools/k1_ab_libs.py)
LIB_PATH = os.environ.get("PROTSTRUC_AMD_LIB") or os.path.join(_HERE, "lib", "libprotstruc_hip.so")
EXPECTED_ABI = 16  # PS_ABI_VERSION of include/protstruc_hip.h; bumped together with any signature change


# the structs that cross the boundary: their layouts are the typedefs of the headers, read from them
class K1Config(ctypes.Structure):
    _fields_ = struct_fields("protstruc_hip.h", "ps_k1_config")


class K1Plan(ctypes.Structure):
    _fields_ = struct_fields("protstruc_hip.h", "ps_k1_plan")


class K3Plan(ctypes.Structure):
    _fields_ = struct_fields("protstruc_hip.h", "ps_k3_plan")


class SuperposeObjective(ctypes.Structure):
    _fields_ = struct_fields("protstruc_superpose.h", "ps_superpose_objective")


# name -> (restype, argtypes) of every entry point include/protstruc_hip.h declares; a pointer of any kind is a c_void_p
SIGNATURES = prototypes("protstruc_hip.h")

# ---- the side headers: one family of entry points each ------------------------------------------------------------------
# A family is declared in a header of its own with a version of its own (``PS_<FAMILY>_API``, returned by
# ``ps_<family>_api()``), so that adding it changes neither PS_ABI_VERSION nor any earlier declaration.  Here it is its
# header, one line of FAMILIES and an expected version; the table is read from the header, and ``load()`` and
# ``build._deps()`` take the rest from FAMILIES.


class Family(NamedTuple):
    header: str        # file name under include/
    signatures: str    # module attribute: name -> (restype, argtypes), what the header declares
    version_fn: str    # the entry point that returns the library's version of the header
    expected: str      # module attribute: the version this package binds
    word: str          # what ``load()`` calls the family when it refuses a library


FAMILIES = (   # in load order
    Family("protstruc_contacts.h", "CONTACT_SIGNATURES", "ps_contacts_api", "EXPECTED_CONTACTS_API", "contacts"),
    Family("protstruc_pairhead.h", "PAIRHEAD_SIGNATURES", "ps_pairhead_api", "EXPECTED_PAIRHEAD_API", "pair-head"),
    Family("protstruc_superpose.h", "SUPERPOSE_SIGNATURES", "ps_superpose_api", "EXPECTED_SUPERPOSE_API", "superposition"),
    Family("protstruc_structalign.h", "STRUCTALIGN_SIGNATURES", "ps_structalign_api", "EXPECTED_STRUCTALIGN_API",
           "structure-alignment"),
    Family("protstruc_ensemble.h", "ENSEMBLE_SIGNATURES", "ps_ensemble_api", "EXPECTED_ENSEMBLE_API", "ensemble"),
    Family("protstruc_graph.h", "GRAPH_SIGNATURES", "ps_graph_api", "EXPECTED_GRAPH_API", "radius-graph"),
)

EXPECTED_CONTACTS_API = 1  # PS_CONTACTS_API: the closest-atom entry points (K31 / K32)
EXPECTED_PAIRHEAD_API = 1  # PS_PAIRHEAD_API: the pair-head entry points (K33 - K36)
EXPECTED_SUPERPOSE_API = 1  # PS_SUPERPOSE_API: the superposition entry points (K37 - K40)
EXPECTED_STRUCTALIGN_API = 1  # PS_STRUCTALIGN_API: the structure-alignment entry points (K41 - K44)
EXPECTED_ENSEMBLE_API = 1  # PS_ENSEMBLE_API: the ensemble entry points (K45, K46)
EXPECTED_GRAPH_API = 1  # PS_GRAPH_API: the radius-graph entry points (K47, K48)
# CONTACT_SIGNATURES ... GRAPH_SIGNATURES, the attributes FAMILIES names: what each family's header declares
globals().update({family.signatures: prototypes(family.header) for family in FAMILIES})

_lib = None


def _try_build_in_tree():
    """The .so is a git-ignored build artefact; if it did not travel with the tree, compile it in place
    (hipcc is part of the ROCm image).  Never a fallback to another code path: if this fails, load() raises."""
    from . import build

    if not os.path.exists(build.HIPCC):
        return
    try:
        build.build(force=True, verbose=True)
    except Exception as exc:  # noqa: BLE001 -- reported by the caller as "library missing"
        print(f"[protstruc_amd] in-tree build failed: {exc}", flush=True)


def _bind(lib, signatures):
    for name, (restype, argtypes) in signatures.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = restype
        fn.argtypes = argtypes


def load():
    """Load the shared library once, type every entry point and check every version."""
    global _lib
    if _lib is not None:
        return _lib
    from . import build

    in_tree = os.path.abspath(LIB_PATH) == os.path.abspath(build.LIB_PATH)
    if in_tree and build.is_stale() and not os.environ.get("PROTSTRUC_AMD_NO_AUTOBUILD"):
        # missing, or older than csrc/*.hip / include/*.h: rebuild in place (hipcc is part of the ROCm image).
        # Without hipcc a stale library is refused below rather than loaded.
        _try_build_in_tree()
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} is missing: build it with `python -m protstruc_amd.build` "
            "(hipcc --offload-arch=gfx950). protstruc_amd has no CPU fallback.")
    if in_tree and build.is_stale():
        raise HipLibraryError(
            f"{LIB_PATH} is older than its sources (csrc/*.hip, include/*.h) and could not be rebuilt here: "
            "run `python -m protstruc_amd.build --force` where hipcc is available.")
    lib = ctypes.CDLL(LIB_PATH)
    try:
        lib.ps_abi_version.restype = ctypes.c_int
        abi = lib.ps_abi_version()
    except AttributeError as exc:
        raise HipLibraryError(f"{LIB_PATH} does not export ps_abi_version: not a protstruc_amd library") from exc
    if abi != EXPECTED_ABI:
        raise HipLibraryError(f"{LIB_PATH} has ABI version {abi}, this package binds version {EXPECTED_ABI}: "
                              "rebuild with `python -m protstruc_amd.build --force`")
    _bind(lib, SIGNATURES)
    for family in FAMILIES:   # the tables, the expected versions and LIB_PATH are read from the module now, not at import
        _bind(lib, globals()[family.signatures])
        version, expected = getattr(lib, family.version_fn)(), globals()[family.expected]
        if version != expected:
            raise HipLibraryError(f"{LIB_PATH} has {family.word} API version {version}, this package binds version "
                                  f"{expected}: rebuild with `python -m protstruc_amd.build --force`")
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        msg = load().ps_error_string(code)
        raise HipLibraryError(f"{what} failed: hipError {code} ({msg.decode() if msg else '?'})")


# ---- launch settings: one immutable record per device, on the HOST side ---------------------------------------------
# The library itself is stateless (every launch takes its configuration as an argument).  What the Python shell keeps is
# one record per device: the K1 field values (the autotuner's choice for that device's output buffers, plus whatever a
# test or tool set explicitly), the ps_k1_config struct built from them with its ctypes.byref, and the K3 / featuriser
# arithmetic mode.  A record is built once and never mutated: every change builds a new one under _lock and swaps it
# into _records, so a launch reads its settings with one lock-free dict lookup and a thread that changes a knob can
# never tear the configuration another thread is launching with (the library copies the struct by value).
_K1_KEYS = {   # tuning key -> (struct field, lowest, highest)
    "k1_exact_sqrt": ("exact_sqrt", 0, 1), "k1_variant": ("variant", 0, 1), "k1_flat": ("flat", 0, 4),
    "k1_rows_per_block": ("rows_per_block", 1, 32), "k1_lds_pad_kb": ("lds_pad_kb", -1, 120),
    "k1_flat_cpw": ("flat_cpw", 1, 64), "k1_flat_lds_pad_kb": ("flat_lds_pad_kb", 0, 100),
    "k1_jt": ("jt", 0, 128), "k1_xcd_remap": ("xcd_remap", 0, 1), "k1_store_nt": ("store_nt", 0, 1),
    "k1_flat_fl_log2": ("flat_fl_log2", 0, 7), "k1_rowphase": ("rowphase", 0, 255), "k1_experiment": ("experiment", 0, 31),
}
_lock = threading.RLock()
_records = {}   # device index -> _Record


class _Record(NamedTuple):
    fields: dict        # ps_k1_config field -> value
    cfg: K1Config       # the struct built from ``fields``
    ref: object         # ctypes.byref(cfg): what a launch passes
    exact_angles: int   # 0 fast / 1 the reference's order of operations


def _make_record(fields, exact_angles):
    cfg = K1Config(**fields)
    return _Record(fields, cfg, ctypes.byref(cfg), exact_angles)


def _env_flag(name):
    return 1 if os.environ.get(name, "0") not in ("", "0") else 0


def _device_index(device=None):
    idx = getattr(device, "index", None)     # torch.device with an explicit index: the hot path
    if idx is not None:
        return idx
    if device is None:
        import torch
        return torch.cuda.current_device() if torch.cuda.is_available() else 0
    if isinstance(device, int):
        return device
    import torch
    d = torch.device(device)
    return d.index if d.index is not None else (torch.cuda.current_device() if torch.cuda.is_available() else 0)


def _record(device=None):
    """The current record of ``device``; its first use builds it from ``ps_k1_config_default`` and the environment."""
    idx = _device_index(device)
    rec = _records.get(idx)      # the hit path takes no lock: records are replaced, never mutated
    if rec is None:
        with _lock:
            rec = _records.get(idx)
            if rec is None:
                cfg = K1Config()
                load().ps_k1_config_default(ctypes.byref(cfg))
                fields = {f: getattr(cfg, f) for f, _ in K1Config._fields_}
                # K1 uses the hardware square root (<= 1 ulp) unless the user asks for the correctly rounded one
                if _env_flag("PROTSTRUC_AMD_EXACT_SQRT"):
                    fields["exact_sqrt"] = 1
                rec = _records[idx] = _make_record(fields, _env_flag("PROTSTRUC_AMD_EXACT_ANGLES"))
    return rec


def _checked_field(key, value):
    """(struct field, int value) of one tuning change, or HipLibraryError: every range rule of ``set_tuning``."""
    value = int(value)
    if key not in _K1_KEYS:
        raise HipLibraryError(f"unknown tuning key {key!r} (known: {', '.join(sorted(_K1_KEYS))})")
    field, lo, hi = _K1_KEYS[key]
    if not lo <= value <= hi or (key == "k1_jt" and value not in (0, 16, 32, 64, 128)) \
            or (key == "k1_flat_fl_log2" and value in (1, 2, 3)) or (key == "k1_flat" and value == 3):
        raise HipLibraryError(f"tuning value {key}={value} outside its range")
    if key == "k1_experiment" and value and not load().ps_has_experiments():
        raise HipLibraryError("k1_experiment is reserved and must be 0: the product library contains no timing experiments")
    return field, value


def _change(device, changes):
    """Swap in a record with ``changes`` (tuning keys and / or ``exact_angles``) applied; returns the one it replaced.
    Everything is validated before anything is stored, so a refused change leaves the settings as they were."""
    changes = dict(changes)
    angles = changes.pop("exact_angles", None)
    updates = dict(_checked_field(key, value) for key, value in changes.items())
    with _lock:
        idx = _device_index(device)
        old = _record(idx)
        _records[idx] = _make_record({**old.fields, **updates}, old.exact_angles if angles is None else (1 if angles else 0))
    return old


def set_tuning(key, value, device=None):
    """Set one K1 knob for ``device`` (default: the current device).  Host-side state only."""
    _change(device, {key: value})


def get_tuning(key, device=None):
    if key not in _K1_KEYS:
        raise HipLibraryError(f"unknown tuning key {key!r}")
    return _record(device).fields[_K1_KEYS[key][0]]


def all_tuning(device=None):
    """Every K1 knob of ``device`` as a dict (what ``bench.py`` reports)."""
    fields = _record(device).fields
    return {key: fields[field] for key, (field, _, _) in sorted(_K1_KEYS.items())}


def set_exact_angles(flag, device=None):
    """K3 / featuriser arithmetic mode of ``device`` (the library takes it per call, like exact_sqrt)."""
    _change(device, {"exact_angles": flag})


def get_exact_angles(device=None):
    return _record(device).exact_angles


@contextlib.contextmanager
def scoped_settings(device=None, **changes):
    """Apply ``changes`` -- tuning keys (``k1_jt=16``, ...) and / or ``exact_angles=...`` -- to ``device`` for the
    length of a ``with`` block, through ``set_tuning``'s validation.  On exit, also by an exception, the record that
    was current on entry is put back, which undoes any ``set_tuning`` / ``set_exact_angles`` made inside the block too.
    For tests and tools: the exit overwrites whatever another thread changed on that device in the meantime."""
    idx = _device_index(device)
    old = _change(idx, changes)
    try:
        yield
    finally:
        with _lock:
            _records[idx] = old


def k1_config(device=None, **overrides):
    """Snapshot of ``device``'s K1 configuration as a ``ps_k1_config`` struct (fields overridden by keyword).
    Without overrides the struct is the one of the device's current record: it is never modified in place (a change
    of settings installs a new record), and the library copies it by value before launching, so sharing it between
    launches and threads keeps the snapshot semantics.  With overrides the struct is a fresh one."""
    rec = _record(device)
    return K1Config(**{**rec.fields, **overrides}) if overrides else rec.cfg


def k1_config_ref(idx):
    """``ctypes.byref`` of the configuration struct of device ``idx``'s current record (the launch hot path: one dict
    lookup)."""
    rec = _records.get(idx)
    return (rec if rec is not None else _record(idx)).ref


def row_range(N, row_begin, row_end, compact):
    """K1 / K3 row addressing: (row_end, output rows, origin row) of residue rows [row_begin, row_end) written into a
    compact buffer or into their own rows of a full-size one.  ``row_end`` None means N."""
    row_end = N if row_end is None else row_end
    return (row_end, row_end - row_begin, row_begin) if compact else (row_end, N, 0)


def k1_plan(B, N, A, row_begin=0, row_end=None, *, compact=False, dist_misalign=0, mask_misalign=0, has_atom_mask=True,
            device=None, **overrides):
    """Which kernel ``ps_pairwise_distance_cfg_f32`` takes for this shape under ``device``'s current configuration
    (fields overridden by keyword): a dict with ``family``, ``kernel``, ``n_launches``, ``n_workgroups``, ``lds_bytes``.
    Pure host query (``ps_k1_plan_f32``): the library runs its own dispatcher in record-only mode."""
    row_end, out_rows, origin = row_range(N, row_begin, row_end, compact)
    plan = K1Plan(struct_size=ctypes.sizeof(K1Plan))
    cfg = k1_config(device, **overrides)
    check(load().ps_k1_plan_f32(B, N, A, row_begin, row_end, out_rows, origin, dist_misalign, mask_misalign,
                                int(bool(has_atom_mask)), ctypes.byref(cfg), ctypes.byref(plan)), "ps_k1_plan_f32")
    return {"family": plan.family.decode(), "kernel": plan.kernel.decode(), "n_launches": plan.n_launches,
            "n_workgroups": plan.n_workgroups, "lds_bytes": plan.lds_bytes,
            "threads_per_workgroup": plan.threads_per_workgroup,
            **({"n_workgroups_2": plan.n_workgroups_2, "lds_bytes_2": plan.lds_bytes_2} if plan.n_launches > 1 else {})}


def _k3_plan_dict(plan):
    d = {name: getattr(plan, name) for name, _ in K3Plan._fields_ if name not in ("struct_size", "family", "kernel")}
    d["family"], d["kernel"] = plan.family.decode(), plan.kernel.decode()
    return d


def k3_plan(B, N, A, slots_i, slots_j, n_points, row_begin=0, row_end=None, *, compact=False, out_misalign=0, exact_angles=0,
            cu_count=0):
    """Which kernel ``ps_pairwise_angles_f32`` takes for this launch: a dict with ``family`` ("sweep", "flat_tiles",
    "small", "one_column", "empty"), ``kernel`` (name with template arguments), the layout (``columns_per_lane``,
    ``vector_stores`` -- flat_tiles: 2 = four-column tiles with 16-byte rows, 1 = two-column tiles, 0 = dword stores --,
    ``skips_dead_groups``, ``faithful``), ``rows_per_task``, ``workgroups_per_cu``, grid, workgroup size and LDS bytes.
    Pure host query (``ps_k3_plan_f32``): the library runs its own dispatcher in record-only mode; no GPU needed.
    ``cu_count`` <= 0 means 256 (MI355X)."""
    row_end, out_rows, origin = row_range(N, row_begin, row_end, compact)
    slots = [int(v) for v in slots_i] + [int(v) for v in slots_j]
    src = [0] * len(slots_i) + [1] * len(slots_j)
    arr = ctypes.c_int * n_points
    plan = K3Plan(struct_size=ctypes.sizeof(K3Plan))
    check(load().ps_k3_plan_f32(B, N, A, n_points, arr(*src[:n_points]), arr(*slots[:n_points]), row_begin, row_end, out_rows,
                                origin, out_misalign, int(exact_angles), cu_count, ctypes.byref(plan)), "ps_k3_plan_f32")
    return _k3_plan_dict(plan)


def featuriser_plan(B, N, A=15, *, float_misalign=0, mask_misalign=0, exact_sqrt=0, exact_angles=0, cu_count=0):
    """Which kernel ``ps_inter_residue_geometry_f32`` takes (``ps_featuriser_plan_f32``; see ``k3_plan``)."""
    plan = K3Plan(struct_size=ctypes.sizeof(K3Plan))
    check(load().ps_featuriser_plan_f32(B, N, A, float_misalign, mask_misalign, int(exact_sqrt), int(exact_angles), cu_count,
                                        ctypes.byref(plan)), "ps_featuriser_plan_f32")
    return _k3_plan_dict(plan)
