"""``_headers.prototypes`` and ``_headers.struct_fields`` on header text written for the purpose: what the reader has to
get right in any header, and what it has to refuse.  (That it reads the seven real headers as the bindings typed them by
hand is tests/test_abi_snapshot.py.)  No GPU and no built library needed."""
import ctypes

import pytest

from protstruc_amd import _headers, _lib

SYNTHETIC = """
/* a block comment that calls ps_in_a_comment(int x); and spans
 * lines */
#ifndef SYNTHETIC_H
#define SYNTHETIC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define PS_SYNTHETIC_API 3   /* ps_in_a_macro_comment(void); */
int ps_synthetic_api(void);
// ps_in_a_line_comment(float y);
const char *ps_text(int code);   // trailing ps_trailing(int z);
long long ps_bytes(int B,
                   long long  n,   /* a comment between parameters, with a comma, and ps_inner( */
                   unsigned flags);
void ps_fill(ps_box* box);
double ps_mean(const float* x, float scale, double shift, void* stream);
int ps_make(ps_handle** out, const void *id, const int32_t * table,
            uint64_t*state);
typedef struct ps_box {
    int struct_size;     /* = sizeof(ps_box) */
    char name[24];       // text
    unsigned n; float weight;
    char  tag [ 8 ];
} ps_box;
#ifdef __cplusplus
}
#endif
#endif
"""


@pytest.fixture
def include(tmp_path, monkeypatch):
    monkeypatch.setattr(_headers, "INCLUDE", str(tmp_path))
    (tmp_path / "synthetic.h").write_text(SYNTHETIC)
    return tmp_path


def test_prototypes_of_the_synthetic_header(include):
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _headers.prototypes("synthetic.h") == {
        "ps_synthetic_api": (i, []),                                                 # (void): no parameters
        "ps_text": (ctypes.c_char_p, [i]),                                           # const char *, however it is spaced
        "ps_bytes": (ctypes.c_longlong, [i, ctypes.c_longlong, ctypes.c_uint]),      # over three lines
        "ps_fill": (None, [vp]),                                                     # a pointer to a struct
        "ps_mean": (ctypes.c_double, [vp, ctypes.c_float, ctypes.c_double, vp]),
        "ps_make": (i, [vp, vp, vp, vp]),                                            # T**, and * wherever it stands
    }


def test_struct_fields_of_the_synthetic_header(include):
    fields = _headers.struct_fields("synthetic.h", "ps_box")
    assert fields == [("struct_size", ctypes.c_int), ("name", ctypes.c_char * 24), ("n", ctypes.c_uint),
                      ("weight", ctypes.c_float), ("tag", ctypes.c_char * 8)]
    box = type("Box", (ctypes.Structure,), {"_fields_": fields})
    assert ctypes.sizeof(box) == 4 + 24 + 4 + 4 + 8 and box(name=b"abc").name == b"abc"


@pytest.mark.parametrize("declaration, named", [
    ("int ps_odd(size_t n);", "ps_odd"),                       # a by-value type the reader has no ctypes spelling for
    ("int ps_odd(unsigned int n);", "ps_odd"),
    ("int ps_odd(int);", "ps_odd"),                            # no parameter name: the type cannot be told from it
    ("size_t ps_odd(int n);", "ps_odd"),                       # ... nor for this result
    ("char* ps_odd(int n);", "ps_odd"),                        # only const char* comes back as a string
    ("int ps_odd(int (*callback)(int), int n);", "ps_odd"),    # a declaration the pattern does not cover is not skipped
])
def test_an_unknown_spelling_is_refused_by_name(include, declaration, named):
    (include / "odd.h").write_text("int ps_fine(int n);\n" + declaration + "\n")
    with pytest.raises(_lib.HipLibraryError) as info:
        _headers.prototypes("odd.h")
    assert named in str(info.value) and "odd.h" in str(info.value) and "ps_fine" not in str(info.value)


@pytest.mark.parametrize("field", ["double x;", "int* p;", "int x[4];", "long long n;"])
def test_an_unknown_field_is_refused(include, field):
    (include / "odd.h").write_text("typedef struct ps_odd { int a; %s } ps_odd;\n" % field)
    with pytest.raises(_lib.HipLibraryError, match="ps_odd") as info:
        _headers.struct_fields("odd.h", "ps_odd")
    assert field.rstrip(";") in str(info.value) and "odd.h" in str(info.value)
    with pytest.raises(_lib.HipLibraryError, match="no typedef struct ps_other"):
        _headers.struct_fields("odd.h", "ps_other")


def test_a_missing_header_is_named(include):
    for read in (_headers.prototypes, lambda name: _headers.struct_fields(name, "ps_box")):
        with pytest.raises(_lib.HipLibraryError) as info:
            read("absent.h")
        assert str(include / "absent.h") in str(info.value)


def test_the_headers_are_found_where_the_build_finds_them():
    """relative to the package, as ``build._deps()`` does: the digest of the library covers what the bindings are read from"""
    import os

    from protstruc_amd import build
    for family in _lib.FAMILIES:
        assert os.path.join(_headers.INCLUDE, family.header) in build._deps()
    assert os.path.join(_headers.INCLUDE, "protstruc_hip.h") in build._deps()
