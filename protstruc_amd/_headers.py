"""The C ABI as the headers under include/ state it, read into ctypes terms: ``_lib`` and ``_rccl`` bind what the headers
declare (and the compiler holds the definitions to), so no signature and no struct layout is typed a second time.  A
spelling this reader does not know is an error at import, never a guess."""
import ctypes
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
_BY_VALUE = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
             "long long": ctypes.c_longlong}
_RETURNS = {**_BY_VALUE, "void": None, "const char*": ctypes.c_char_p}


class HipLibraryError(RuntimeError):
    """the one error of the native boundary (``_lib.HipLibraryError``); defined here because reading a header can raise it"""


def _code(header):
    """(path, text without comments and preprocessor lines) of include/``header``"""
    path = os.path.join(INCLUDE, header)
    try:
        with open(path) as f:
            text = f.read()
    except OSError as exc:
        raise HipLibraryError(f"{path} is missing: the bindings are read from the C headers ({exc})") from exc
    return path, re.sub(r"^[ \t]*#.*$", "", re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S), flags=re.M)


def prototypes(header):
    """{name: (restype, [argtypes])} of every ``ps_*`` function include/``header`` declares.  Parameters and results by
    value are int, unsigned, float, double or long long; a result may also be void or ``const char*``; every parameter whose
    type has a ``*`` binds as ``c_void_p``."""
    path, code = _code(header)
    found = {}
    for result, name, parameters in re.findall(r"([^;{}()]*?)\b(ps_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", code):
        result = re.sub(r"\s*\*", "*", " ".join(result.split()))
        parameters = [" ".join(p.split()) for p in parameters.split(",")]
        try:
            found[name] = (_RETURNS[result], [] if parameters == ["void"] else
                           [ctypes.c_void_p if "*" in p else _BY_VALUE[p.rpartition(" ")[0]] for p in parameters])
        except KeyError as exc:
            raise HipLibraryError(f"{path}: cannot bind {result} {name}({', '.join(parameters)}): "
                                  f"no ctypes spelling for {exc.args[0]!r}") from None
    unread = sorted(set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", code)) - set(found))
    if unread:
        raise HipLibraryError(f"{path}: cannot read the declaration of {', '.join(unread)}")
    return found


def struct_fields(header, name):
    """the ``_fields_`` list of ``typedef struct name { ... } name;`` in include/``header``: int, unsigned and float fields
    and ``char x[N]``"""
    path, code = _code(header)
    body = re.search(r"typedef\s+struct\s+%s\s*\{([^{}]*)\}\s*%s\s*;" % (name, name), code)
    if body is None:
        raise HipLibraryError(f"{path}: no typedef struct {name}")
    fields = []
    for declaration in filter(None, (" ".join(d.split()) for d in body.group(1).split(";"))):
        scalar = re.fullmatch(r"(int|unsigned|float) (\w+)", declaration)
        text = re.fullmatch(r"char (\w+) ?\[ ?(\d+) ?\]", declaration)
        if not scalar and not text:
            raise HipLibraryError(f"{path}: cannot bind struct {name}: no ctypes spelling for {declaration!r}")
        fields.append((scalar.group(2), _BY_VALUE[scalar.group(1)]) if scalar else (text.group(1), ctypes.c_char * int(text.group(2))))
    return fields
