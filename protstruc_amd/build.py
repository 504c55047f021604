"""Build libprotstruc_hip.so (and the libraries beside it) for gfx950 with hipcc (cross-compiles without a GPU).

    python -m protstruc_amd.build [--force]

The library is built IN-TREE (protstruc_amd/lib/) so that it travels with the
repository snapshot to the GPU box; nothing is JIT-compiled at import time.
-ffp-contract=off is part of the numerical contract (see csrc/ps_common.hpp).
"""
import glob
import hashlib
import os
import subprocess
import sys
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libprotstruc_hip.so")
# the multi-GPU exchange step lives in its own library so that libprotstruc_hip.so has no RCCL dependency
RCCL_SRC_DIR = os.path.join(HERE, "csrc_rccl")
RCCL_LIB_PATH = os.path.join(LIB_DIR, "libprotstruc_rccl.so")
# the edge features on CSR graphs (K49 - K51) are a library of their own, with a header and a version of their own:
# include/protstruc_csredge.h
CSREDGE_SRC_DIR = os.path.join(HERE, "csrc_csredge")
CSREDGE_LIB_PATH = os.path.join(LIB_DIR, "libprotstruc_csredge.so")
# the backward kernels of the edge features (K52 - K54), likewise: include/protstruc_edgegrad.h
EDGEGRAD_SRC_DIR = os.path.join(HERE, "csrc_edgegrad")
EDGEGRAD_LIB_PATH = os.path.join(LIB_DIR, "libprotstruc_edgegrad.so")
# message passing on graphs (K55 - K59), likewise: include/protstruc_aggregate.h
AGGREGATE_SRC_DIR = os.path.join(HERE, "csrc_aggregate")
AGGREGATE_LIB_PATH = os.path.join(LIB_DIR, "libprotstruc_aggregate.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ROCM_LIB = os.environ.get("ROCM_LIB", "/opt/rocm/lib")
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared"]


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def _deps():
    """Everything the library is compiled from: the sources and the public headers, protstruc_hip.h and one per family
    of ``_lib.FAMILIES`` (protstruc_rccl.h belongs to the other library)."""
    from ._lib import FAMILIES
    return sources() + sorted(glob.glob(os.path.join(CSRC, "*.hpp"))) + \
        [os.path.join(HERE, "..", "include", name) for name in ["protstruc_hip.h"] + [family.header for family in FAMILIES]]


class _Target(NamedTuple):
    """One native product with the digest of what it was built from recorded beside it (``out`` + ".srchash"): built only
    when that digest is not the tree's, aside under a pid-suffixed name and renamed into place, so that concurrent builders
    (one per rank) cannot corrupt it."""
    out: str          # the file that is built
    seed: bytes       # what the digest starts from
    inputs: list      # the files the digest covers, in this order, each by base name and contents
    command: object   # path to write -> the compiler's command line

    def digest(self):
        h = hashlib.sha256(self.seed)
        for d in self.inputs:
            h.update(os.path.basename(d).encode())
            with open(d, "rb") as f:
                h.update(f.read())
        return h.hexdigest()

    def is_stale(self):
        """True when ``out`` is missing or was built from other inputs than the ones in the tree now.  Compared by
        content digest, not by mtime: a snapshot copied to another machine keeps its contents but not necessarily its
        timestamps."""
        if not os.path.exists(self.out):
            return True
        try:
            with open(self.out + ".srchash") as f:
                return f.read().strip() != self.digest()
        except OSError:
            return True

    def build(self, force, verbose):
        if not force and not self.is_stale():
            return self.out
        os.makedirs(os.path.dirname(self.out), exist_ok=True)
        tmp = f"{self.out}.{os.getpid()}.tmp"
        cmd = self.command(tmp)
        if verbose:
            print("[protstruc_amd.build]", " ".join(cmd), flush=True)
        try:
            digest = self.digest()
            subprocess.run(cmd, check=True)
            os.replace(tmp, self.out)
            with open(self.out + ".srchash", "w") as f:
                f.write(digest + "\n")
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        return self.out


def _library(out=None):
    return _Target(out or LIB_PATH, " ".join(FLAGS).encode(), _deps(), lambda tmp: [HIPCC] + FLAGS + ["-o", tmp] + sources())


def source_hash():
    """Digest of everything the library is compiled from (file names, contents, flags)."""
    return _library().digest()


def is_stale(path=None):
    """Whether the library at ``path`` (default: the tree's) has to be built: see ``_Target.is_stale``."""
    return _library(path).is_stale()


def build(force=False, verbose=True):
    return _library().build(force, verbose)


build_graph = build   # transitional, see _graph.py: the radius graph's former build step; unused, deleted with that module


def rccl_sources():
    return sorted(glob.glob(os.path.join(RCCL_SRC_DIR, "*.cpp")))


def _rccl_library():
    return _Target(RCCL_LIB_PATH, b"rccl-lib-v1", rccl_sources() + [os.path.join(HERE, "..", "include", "protstruc_rccl.h")],
                   lambda tmp: [HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp] + rccl_sources() +
                   ["-L" + ROCM_LIB, "-lrccl", "-Wl,-rpath," + ROCM_LIB])


def rccl_is_stale():
    return _rccl_library().is_stale()


def build_rccl(force=False, verbose=True):
    """libprotstruc_rccl.so: host-only C++ over RCCL (ps_allgather_rows, include/protstruc_rccl.h).  Linked against
    librccl.so.1 by SONAME: inside a PyTorch process that is the RCCL PyTorch already loaded, so one copy serves both."""
    return _rccl_library().build(force, verbose)


def csredge_sources():
    return sorted(glob.glob(os.path.join(CSREDGE_SRC_DIR, "*.hip")))


def _csredge_library(out=None):
    inputs = csredge_sources() + sorted(glob.glob(os.path.join(CSREDGE_SRC_DIR, "*.hpp"))) + \
        sorted(glob.glob(os.path.join(CSRC, "*.hpp"))) + [os.path.join(HERE, "..", "include", "protstruc_csredge.h")]
    return _Target(out or CSREDGE_LIB_PATH, b"csredge-lib " + " ".join(FLAGS).encode(), inputs,
                   lambda tmp: [HIPCC] + FLAGS + ["-I" + CSRC, "-o", tmp] + csredge_sources())


def csredge_is_stale(path=None):
    return _csredge_library(path).is_stale()


def build_csredge(force=False, verbose=True):
    """libprotstruc_csredge.so: csrc_csredge/*.hip, the edge features on CSR graphs (include/protstruc_csredge.h).  Compiled
    with exactly FLAGS and -I csrc: the kernels share ps_common.hpp with libprotstruc_hip.so and its arithmetic contract
    (-ffp-contract=off), and add no export to it."""
    return _csredge_library().build(force, verbose)


def edgegrad_sources():
    return sorted(glob.glob(os.path.join(EDGEGRAD_SRC_DIR, "*.hip")))


def _edgegrad_library(out=None):
    inputs = edgegrad_sources() + sorted(glob.glob(os.path.join(EDGEGRAD_SRC_DIR, "*.hpp"))) + \
        sorted(glob.glob(os.path.join(CSRC, "*.hpp"))) + [os.path.join(HERE, "..", "include", "protstruc_edgegrad.h")]
    return _Target(out or EDGEGRAD_LIB_PATH, b"edgegrad-lib " + " ".join(FLAGS).encode(), inputs,
                   lambda tmp: [HIPCC] + FLAGS + ["-I" + CSRC, "-o", tmp] + edgegrad_sources())


def edgegrad_is_stale(path=None):
    return _edgegrad_library(path).is_stale()


def build_edgegrad(force=False, verbose=True):
    """libprotstruc_edgegrad.so: csrc_edgegrad/*.hip, the backward kernels of the edge features
    (include/protstruc_edgegrad.h).  Compiled with exactly FLAGS and -I csrc, like libprotstruc_csredge.so, and for the same
    reason: it shares ps_common.hpp and -ffp-contract=off with the forward kernels, and adds no export to them."""
    return _edgegrad_library().build(force, verbose)


def aggregate_sources():
    return sorted(glob.glob(os.path.join(AGGREGATE_SRC_DIR, "*.hip")))


def _aggregate_library(out=None):
    inputs = aggregate_sources() + sorted(glob.glob(os.path.join(AGGREGATE_SRC_DIR, "*.hpp"))) + \
        sorted(glob.glob(os.path.join(CSRC, "*.hpp"))) + [os.path.join(HERE, "..", "include", "protstruc_aggregate.h")]
    return _Target(out or AGGREGATE_LIB_PATH, b"aggregate-lib " + " ".join(FLAGS).encode(), inputs,
                   lambda tmp: [HIPCC] + FLAGS + ["-I" + CSRC, "-o", tmp] + aggregate_sources())


def aggregate_is_stale(path=None):
    return _aggregate_library(path).is_stale()


def build_aggregate(force=False, verbose=True):
    """libprotstruc_aggregate.so: csrc_aggregate/*.hip, message passing on graphs -- segment reductions, gathers and the edge
    softmax (include/protstruc_aggregate.h).  Compiled with exactly FLAGS and -I csrc, like libprotstruc_edgegrad.so, and for
    the same reason: it shares ps_common.hpp and -ffp-contract=off with the other kernels, and adds no export to them."""
    return _aggregate_library().build(force, verbose)


EXAMPLE_SRC = os.path.join(HERE, "..", "examples", "c_abi_demo.c")
EXAMPLE_BIN = os.path.join(HERE, "..", "build", "c_abi_demo")


def build_c_example(verbose=True):
    """examples/c_abi_demo.c with plain gcc -std=c99: proves that include/protstruc_hip.h is a C header and that the
    boundary needs neither C++ nor PyTorch on the caller's side.  The binary is a GPU test (tests/test_c_abi_from_c.py)."""
    os.makedirs(os.path.dirname(EXAMPLE_BIN), exist_ok=True)
    rocm_inc = os.path.join(os.path.dirname(ROCM_LIB.rstrip("/")), "include")
    cmd = ["gcc", "-std=c99", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
           "-I" + rocm_inc, "-I" + os.path.join(HERE, "..", "include"), EXAMPLE_SRC,
           "-L" + LIB_DIR, "-lprotstruc_hip", "-L" + ROCM_LIB, "-lamdhip64", "-lm",
           "-Wl,-rpath,$ORIGIN/../protstruc_amd/lib", "-Wl,-rpath," + ROCM_LIB, "-o", EXAMPLE_BIN]
    if verbose:
        print("[protstruc_amd.build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return EXAMPLE_BIN


PROBE_SRC = os.path.join(HERE, "..", "tests", "native", "arith_probe.hip")
PROBE_LIB_PATH = os.path.join(HERE, "..", "build", "libps_arith_probe.so")


def _arith_probe():
    return _Target(PROBE_LIB_PATH, " ".join(FLAGS).encode(), [PROBE_SRC] + sorted(glob.glob(os.path.join(CSRC, "*.hpp"))),
                   lambda tmp: [HIPCC] + FLAGS + ["-I" + CSRC, "-o", tmp, PROBE_SRC])


def arith_probe_is_stale():
    return _arith_probe().is_stale()


def build_arith_probe(force=False, verbose=True):
    """build/libps_arith_probe.so: tests/native/arith_probe.hip, the test-only entry point that evaluates one arithmetic
    primitive of csrc/*.hpp elementwise (tests/test_gpu_arith.py).  Compiled with exactly FLAGS -- the primitives must be
    probed in the arithmetic the library runs them in -- and kept out of libprotstruc_hip.so: the product ABI has no probe."""
    return _arith_probe().build(force, verbose)


if __name__ == "__main__":
    force = "--force" in sys.argv
    print(build(force=force))
    print(build_rccl(force=force))
    print(build_csredge(force=force))
    print(build_edgegrad(force=force))
    print(build_aggregate(force=force))
    print(build_c_example())
    print(build_arith_probe(force=force))
