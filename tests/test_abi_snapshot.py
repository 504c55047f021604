"""The whole C boundary as the bindings type it, held to a committed snapshot (tests/golden/abi_snapshot.json): every entry
point of the eight headers with its return class and its parameter classes, and the four structs the bindings mirror with
their field names, field types and ``ctypes.sizeof``.  The snapshot was written from the hand-typed tables the bindings had
before they read the headers, so it checks the header reader independently, and any later change of the ABI shows in its
diff.  ``python -m tests.test_abi_snapshot`` rewrites it -- only ever together with the header change that it records.
No GPU and no built library needed."""
import ctypes
import json
import os

from protstruc_amd import _lib, _rccl

SNAPSHOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_snapshot.json")
TABLES = {"protstruc_hip.h": _lib.SIGNATURES, "protstruc_rccl.h": _rccl.SIGNATURES,
          **{family.header: getattr(_lib, family.signatures) for family in _lib.FAMILIES}}
STRUCTS = {"ps_k1_config": _lib.K1Config, "ps_k1_plan": _lib.K1Plan, "ps_k3_plan": _lib.K3Plan,
           "ps_superpose_objective": _lib.SuperposeObjective}
SCALARS = {None: "void", ctypes.c_char_p: "str", ctypes.c_void_p: "ptr", ctypes.c_int: "int", ctypes.c_uint: "uint",
           ctypes.c_float: "float", ctypes.c_double: "double", ctypes.c_longlong: "longlong"}


def type_class(ctype):
    """``c_void_p`` and every ``POINTER(x)`` are "ptr"; a type the snapshot has no word for is a KeyError"""
    if isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer):
        return "ptr"
    if isinstance(ctype, type) and issubclass(ctype, ctypes.Array):
        assert ctype._type_ is ctypes.c_char
        return f"char[{ctype._length_}]"
    return SCALARS[ctype]


def live():
    """one string per entry point, ``int(ptr, int, float)``, and per struct field, ``name: type``"""
    return {"functions": {header: {name: f"{type_class(restype)}({', '.join(type_class(arg) for arg in argtypes)})"
                                   for name, (restype, argtypes) in table.items()}
                          for header, table in TABLES.items()},
            "structs": {name: {"sizeof": ctypes.sizeof(cls), "fields": [f"{field}: {type_class(ctype)}" for field, ctype in cls._fields_]}
                        for name, cls in STRUCTS.items()}}


def test_the_bindings_are_the_snapshot():
    with open(SNAPSHOT) as f:
        want = json.load(f)
    got = live()
    assert sorted(got["functions"]) == sorted(want["functions"])
    for header, table in want["functions"].items():
        assert sorted(got["functions"][header]) == sorted(table), header
        for name, signature in table.items():
            assert got["functions"][header][name] == signature, (header, name)
    assert got["structs"] == want["structs"]
    assert sum(len(table) for table in want["functions"].values()) == 92 and len(want["structs"]) == 4


if __name__ == "__main__":
    with open(SNAPSHOT, "w") as f:
        json.dump(live(), f, indent=1, sort_keys=True)
        f.write("\n")
