"""Transitional: the names of the radius graph's former loader.  K47 and K48 are a family of libprotstruc_hip.so
(``_lib.FAMILIES``, include/protstruc_graph.h) and ``_lib.load()`` is the only loader; nothing in the package or its tests
uses this module.  It stays for one commit, so that what was written against the separate library the commit before still
imports, and is deleted with ``build.build_graph`` after that."""
from ._lib import EXPECTED_GRAPH_API as EXPECTED_API, GRAPH_SIGNATURES as SIGNATURES, LIB_PATH, check, load  # noqa: F401
