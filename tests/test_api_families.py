"""The side headers of the C ABI, one family of entry points each, held to ``_lib.FAMILIES`` without a GPU: every header is
C99, declares exactly what its binding table types and what the cross-compiled library exports, carries the version the
binding expects, and is a dependency of the build; no name is in two tables; a library with another version of any family
is refused in that family's words.  A second table holds every constant of ``ops`` whose comment names a ``PS_*`` macro to
the header it names.  What is a family's own -- its launchers, its refusals, its yardsticks -- is in tests/test_*_host.py."""
import ctypes
import os
import re
import subprocess

import pytest

from protstruc_amd import _lib, build, ops
from tests.c_headers import INCLUDE, declared_symbols, header_text, macros

FAMILIES = pytest.mark.parametrize("family", _lib.FAMILIES, ids=[family.word for family in _lib.FAMILIES])
TABLES = ["SIGNATURES"] + [family.signatures for family in _lib.FAMILIES]


@pytest.fixture(scope="module")
def lib():
    build.build(force=False, verbose=False)      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_the_registry_is_the_six_families_in_load_order():
    assert [family.word for family in _lib.FAMILIES] == ["contacts", "pair-head", "superposition", "structure-alignment",
                                                         "ensemble", "radius-graph"]
    for family in _lib.FAMILIES:
        stem = re.fullmatch(r"ps_([a-z]+)_api", family.version_fn).group(1)
        assert family.header == f"protstruc_{stem}.h" and family.expected == f"EXPECTED_{stem.upper()}_API"
        assert isinstance(getattr(_lib, family.signatures), dict) and isinstance(getattr(_lib, family.expected), int)
        assert family.version_fn in getattr(_lib, family.signatures)


@FAMILIES
def test_header_is_c99(family):
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(INCLUDE, family.header)],
                   check=True)


@FAMILIES
def test_header_binding_and_library_agree(family, lib):
    declared, table = declared_symbols(family.header), getattr(_lib, family.signatures)
    assert declared == sorted(table)
    raw = ctypes.CDLL(build.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} is declared in include/{family.header} but not exported"
    # and nothing else is exported: what no other table binds is what this header declares
    nm = subprocess.run(["nm", "-D", "--defined-only", build.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(ps_[a-z0-9_]+)$", nm, flags=re.M))
    others = set().union(*(getattr(_lib, other) for other in TABLES if other != family.signatures))
    assert sorted(exported - others) == declared
    api = macros(family.header)[f"PS_{family.expected[len('EXPECTED_'):]}"]
    assert getattr(lib, family.version_fn)() == api == getattr(_lib, family.expected)
    assert family.header in {os.path.basename(d) for d in build._deps()}


def test_no_name_is_in_two_tables(lib):
    for k, one in enumerate(TABLES):
        for other in TABLES[k + 1:]:
            assert not set(getattr(_lib, one)) & set(getattr(_lib, other)), (one, other)
    assert _lib.EXPECTED_ABI == 16 and lib.ps_abi_version() == 16, "a family leaves PS_ABI_VERSION as it was"
    deps = {os.path.basename(d) for d in build._deps()}
    assert "protstruc_hip.h" in deps and "protstruc_rccl.h" not in deps


@FAMILIES
def test_a_library_with_another_version_is_refused(family, lib, monkeypatch):
    bound = getattr(_lib, family.expected)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, family.expected, bound + 1)
    with pytest.raises(_lib.HipLibraryError) as info:
        _lib.load()
    assert str(info.value) == (f"{_lib.LIB_PATH} has {family.word} API version {bound}, this package binds version {bound + 1}: "
                               "rebuild with `python -m protstruc_amd.build --force`")


# ---- the constants ``ops`` mirrors -----------------------------------------------------------------------------------------------
def mirrored_constants():
    """(name, macro, header) of every module-level constant of ops.py whose comment starts with a ``PS_*`` macro; the header
    is the one the comment names ("PS_X of include/protstruc_y.h"), or the one the constant above it named"""
    rows, header = [], None
    for line in open(ops.__file__):
        found = re.match(r"([A-Z][A-Z0-9_]*) = [^#]+#\s*(PS_[A-Z0-9_]+)(?: of include/(protstruc_[a-z]+\.h))?", line)
        if found:
            header = found.group(3) or header
            rows.append((found.group(1), found.group(2), header))
    return rows


MIRRORED = mirrored_constants()
IN_WORDS = [("IRG_BACKWARD_MAX_N", "protstruc_hip.h", "N <= {}")]   # limits a header states in a sentence, not as a macro


def test_the_table_of_mirrored_constants_is_complete():
    names = {name for name, _, _ in MIRRORED}
    assert {"RNG_STATE_WORDS", "FAPE_FRAME_TILE", "LDDT_MAX_THRESHOLDS", "LDDT_MAX_THRESHOLD", "PEPTIDE_BOND_CONSTANTS",
            "DSSP_MAX_RESIDUES", "SASA_MAX_SPHERE_POINTS", "KNN_MAX_K", "EDGE_MAX_PAIRS", "EDGE_MAX_RBF", "CHI_MAX_TYPES",
            "CLOSEST_MAX_ATOMS", "CLOSEST_MAX_RESIDUES", "PAIRHEAD_MAX_RESIDUES", "PAIRHEAD_MAX_BREAKS", "PAIRHEAD_MAX_BINS",
            "PAIRHEAD_MAX_TABLES", "PAIRHEAD_NO_TARGET", "SUPERPOSE_MAX_POINTS", "SUPERPOSE_MAX_OBJECTIVES", "SUPERPOSE_TM",
            "SUPERPOSE_COUNT", "STRUCTALIGN_MAX_POINTS", "CLUSTER_MAX_ITEMS", "RMSD_MATRIX_MAX_POINTS",
            "RADIUS_TILE", "RADIUS_BOX_FLOATS", "RADIUS_STATS"} <= names
    assert all(macro == "PS_" + name for name, macro, _ in MIRRORED), "a constant is called what its macro is called"


@pytest.mark.parametrize("name, macro, header", MIRRORED, ids=[row[0] for row in MIRRORED])
def test_constant_is_the_macro_of_the_header_it_names(name, macro, header):
    value, want = getattr(ops, name), macros(header)[macro]
    assert value == want and type(value) is type(want), (name, value, want)


@pytest.mark.parametrize("name, header, sentence", IN_WORDS, ids=[row[0] for row in IN_WORDS])
def test_constant_is_what_the_header_says_in_words(name, header, sentence):
    assert sentence.format(getattr(ops, name)) in header_text(header)


def test_known_values_of_the_limits():
    """the values themselves, where a kernel's layout depends on them"""
    assert ops.CLUSTER_MAX_ITEMS == 4096 and ops.RMSD_MATRIX_MAX_POINTS == 2 ** 31 - 1 - 16
    assert ops.CLOSEST_MAX_RESIDUES == ops.PAIRHEAD_MAX_RESIDUES == 2 ** 20 and ops.PAIRHEAD_NO_TARGET == 255
