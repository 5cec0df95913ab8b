"""Builds the native libraries in-tree (no JIT cache, no hipify):

* ``flink_ml_amd/ops/_lib/libfmlx_kernels.so`` — every ``csrc/*.hip`` compiled by hipcc for
  gfx950 and linked into one shared object with a flat ``extern "C"`` launcher API.
* ``flink_ml_amd/ops/_lib/libfmlx_host.so`` — host-side C++ runtime pieces (``csrc/host/*.cpp``:
  murmur3/Java-compatible hashing, data cache, quantile sketches, ...), built with g++.

Staleness is decided by CONTENT, not mtimes: ``_lib/build_manifest.json`` records the sha256
of every source, header, compile flag set and compiler version an object was built from, and
which objects the last build compiled vs reused. ``FMLX_FORCE_BUILD=1`` (or ``--force``)
recompiles everything. At load time ``native`` compares the manifest's source digest with the
tree and refuses a library built from other sources (a stale binary shipped with the tree).

The manifest also carries each library's ``api``: the ctypes signature of every entry point,
parsed from the C definitions marked ``FMLX_API`` (``api_signatures``). ``native`` binds the
libraries' functions from it, so the C prototypes are the only description of the ABI.

``--sanitize``: the host runtime rebuilt with ``-fsanitize=address,undefined`` into
``_lib/libfmlx_host_asan.so`` (the CPU test-suite runs the host paths against it, see
``tests/test_native_build.py``); GPU code is never built with sanitizers.

Usage: ``python -m flink_ml_amd.ops.build [--force] [--sanitize] [-j N]``.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import glob
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "_lib")
OBJDIR = os.path.join(HERE, "_build")
KERNEL_LIB = os.path.join(LIBDIR, "libfmlx_kernels.so")
HOST_LIB = os.path.join(LIBDIR, "libfmlx_host.so")
HOST_ASAN_LIB = os.path.join(LIBDIR, "libfmlx_host_asan.so")
MANIFEST = os.path.join(LIBDIR, "build_manifest.json")
ARCH = os.environ.get("FMLX_OFFLOAD_ARCH", "gfx950")
SANITIZE_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def _sha(path: str) -> str:
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _digest(parts) -> str:
    h = hashlib.sha256()
    for p in parts:
        h.update(str(p).encode())
        h.update(b"\0")
    return h.hexdigest()


def kernel_sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip"))), sorted(glob.glob(os.path.join(CSRC, "*.h")))


def host_sources():
    return sorted(glob.glob(os.path.join(CSRC, "host", "*.cpp"))), sorted(glob.glob(os.path.join(CSRC, "host", "*.h")))


def source_digest(which: str) -> str:
    """sha256 over the (relative name, content hash) of every source of a library."""
    srcs, hdrs = kernel_sources() if which == "kernels" else host_sources()
    return _digest([(os.path.relpath(f, CSRC), _sha(f)) for f in srcs + hdrs])


# The ctypes signature of every entry point is derived from its C definition: a function is an
# entry point iff its definition carries API_MARKER (csrc/common.h, csrc/host/api.h), and these are
# all the parameter / return types one may use (values: attribute names of ``ctypes``). Every
# pointer is a c_void_p (takes an address, None, bytes or a ctypes array); ``void`` returns None.
API_MARKER = "FMLX_API"
C_TYPES = {
    "int": "c_int", "int32_t": "c_int",
    "unsigned": "c_uint", "unsigned int": "c_uint", "uint32_t": "c_uint",
    "long": "c_int64", "long long": "c_int64", "int64_t": "c_int64",
    "unsigned long": "c_uint64", "unsigned long long": "c_uint64", "uint64_t": "c_uint64", "size_t": "c_uint64",
    "float": "c_float",
    "double": "c_double",
}
_TYPE_WORDS = {"void", "char", "short", "int", "long", "signed", "unsigned", "float", "double", "bool"}
# string and character literals (matched so that a "//" inside one opens no comment), comments
_NOT_CODE = re.compile(r'"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'|//[^\n]*|/\*.*?\*/', re.S)
_MARKED = re.compile(r"%s\b([^(){};]*?)(\w+)\s*\(" % API_MARKER)  # marker, return type, name, "("


def _c_type(decl: str, named: bool, what: str):
    """ctypes name of one C parameter declaration (``named``: may end in the parameter's name) or
    return type; raises for anything that is not in C_TYPES: never a guess."""
    if not re.search(r"[^\w\s*]", decl):
        if "*" in decl:
            return "c_void_p"
        words = [w for w in decl.split() if w not in ("const", "__restrict__")]
        if not named and words == ["void"]:
            return None
        if named and len(words) > 1 and words[-1] not in _TYPE_WORDS and " ".join(words) not in C_TYPES:
            words.pop()  # the parameter's name
        if " ".join(words) in C_TYPES:
            return C_TYPES[" ".join(words)]
    raise ValueError("%s: C type '%s' has no ctypes mapping (ops/build.py C_TYPES)" % (what, " ".join(decl.split())))


def parse_api(text: str, where: str, api: dict = None) -> dict:
    """Adds ``{name: (restype, [argtype, ...])}`` of every API_MARKER function in the C/HIP source
    ``text`` (``where``: its file name, for error messages) to ``api`` and returns it."""
    api = {} if api is None else api
    text = _NOT_CODE.sub(" ", text)
    for marker in re.finditer(r"\b%s\b" % API_MARKER, text):
        m = _MARKED.match(text, marker.start())
        if m is None:
            raise ValueError("%s: %s is not followed by 'type name(parameters)'" % (where, API_MARKER))
        name, what = m.group(2), "%s in %s" % (m.group(2), where)
        end = text.find(")", m.end())
        params = text[m.end():end]
        if end < 0 or "(" in params:
            raise ValueError("%s: cannot read the parameter list" % what)
        if name in api:
            raise ValueError("%s: entry point defined twice" % what)
        plist = [] if params.strip() in ("", "void") else params.split(",")
        api[name] = (_c_type(m.group(1), False, what), [_c_type(p, True, what) for p in plist])
    return api


def api_signatures(which: str) -> dict:
    """``{name: (restype, [argtype, ...])}`` (ctypes attribute names; restype None: void) of every
    entry point of the library ``which`` ("kernels" / "host"), parsed from its sources."""
    srcs, _ = kernel_sources() if which == "kernels" else host_sources()
    api = {}
    for path in srcs:
        with open(path) as f:
            parse_api(f.read(), os.path.relpath(path, CSRC), api)
    return api


def _load_manifest() -> dict:
    try:
        with open(MANIFEST) as f:
            return json.load(f)
    except (OSError, ValueError):
        return {}


def _save_manifest(m: dict) -> None:
    tmp = MANIFEST + ".tmp"
    with open(tmp, "w") as f:
        json.dump(m, f, indent=1, sort_keys=True)
    os.replace(tmp, MANIFEST)


def _tool_version(tool: str) -> str:
    try:
        return subprocess.run([tool, "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout.strip()
    except OSError:
        return "?"


def _force(force: bool) -> bool:
    return force or os.environ.get("FMLX_FORCE_BUILD", "0") == "1"


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def _newer(target: str, deps) -> bool:
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def _run(cmd):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("command failed (%d): %s\n%s" % (p.returncode, " ".join(cmd), p.stdout))
    return p.stdout


# per-source compiler options. kmeans.hip: MFMA accumulators in arch VGPRs — its epilogue reads
# every accumulator with VALU ops each tile, and the AGPR form adds a v_accvgpr_read per value.
FILE_FLAGS = {"kmeans.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-Wno-inline-asm"],
              # the fused round's ticket atomics: no lane-0 result fix-up (keeps counted vmcnt waits)
              "glm.hip": ["-mllvm", "-amdgpu-atomic-optimizer-strategy=None"],
              "glm_sparse.hip": ["-mllvm", "-amdgpu-atomic-optimizer-strategy=None"],
              # MFMA accumulators in arch VGPRs: the AGPR form rotated the DCT's accumulators
              # through VGPRs every k step
              "dct.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"]}


def build_kernels(force: bool = False, jobs: int = 8, verbose: bool = False) -> str:
    force = _force(force)
    os.makedirs(LIBDIR, exist_ok=True)
    os.makedirs(OBJDIR, exist_ok=True)
    srcs, headers = kernel_sources()
    hipcc = _hipcc()
    flags = ["--offload-arch=%s" % ARCH, "-O3", "-std=c++17", "-fPIC", "-mcode-object-version=5",
             "-Wno-unused-result", "-I", CSRC]
    man = _load_manifest()
    kman = man.get("kernels", {})
    old_objs = kman.get("objects", {})
    hdr_digest = _digest([_sha(h) for h in headers])
    ver = _tool_version(hipcc)
    objs, todo, keys = [], [], {}
    for s in srcs:
        name = os.path.basename(s)
        o = os.path.join(OBJDIR, name[:-4] + ".o")
        objs.append(o)
        key = _digest([_sha(s), hdr_digest, flags, FILE_FLAGS.get(name, []), ver])
        keys[name] = key
        if force or not os.path.exists(o) or old_objs.get(name) != key:
            todo.append((s, o))

    def comp(so):
        s, o = so
        if verbose:
            print("[hipcc] %s" % os.path.basename(s), flush=True)
        _run([hipcc] + flags + FILE_FLAGS.get(os.path.basename(s), []) + ["-c", s, "-o", o])
        return o

    if todo:
        with cf.ThreadPoolExecutor(max_workers=max(1, jobs)) as ex:
            list(ex.map(comp, todo))
    digest = source_digest("kernels")
    relink = force or bool(todo) or not os.path.exists(KERNEL_LIB) or kman.get("source_digest") != digest
    if relink:
        _run([hipcc, "--offload-arch=%s" % ARCH, "-shared", "-fPIC", "-o", KERNEL_LIB] + objs)
    man = _load_manifest()
    man["kernels"] = {"objects": keys, "source_digest": digest, "api": api_signatures("kernels"), "arch": ARCH,
                      "compiler": ver.splitlines()[0] if ver else "?",
                      "compiled": sorted(os.path.basename(s) for s, _ in todo),
                      "reused": sorted(n for n in keys if n not in {os.path.basename(s) for s, _ in todo}),
                      "linked": relink, "forced": force, "time": time.strftime("%Y-%m-%dT%H:%M:%S")}
    _save_manifest(man)
    return KERNEL_LIB


def build_host(force: bool = False, verbose: bool = False, sanitize: bool = False) -> str:
    force = _force(force)
    os.makedirs(LIBDIR, exist_ok=True)
    srcs, hdrs = host_sources()
    if not srcs:
        return ""
    target = HOST_ASAN_LIB if sanitize else HOST_LIB
    section = "host_asan" if sanitize else "host"
    cxx = os.environ.get("CXX", "g++")
    flags = ["-O1" if sanitize else "-O3", "-std=c++17", "-fPIC", "-shared", "-march=x86-64-v2"] + (
        SANITIZE_FLAGS if sanitize else [])
    digest = source_digest("host")
    key = _digest([digest, flags, _tool_version(cxx)])
    man = _load_manifest()
    if not force and os.path.exists(target) and man.get(section, {}).get("key") == key:
        man[section]["compiled"] = False
        _save_manifest(man)
        return target
    if verbose:
        print("[g++] host runtime%s (%d files)" % (" (ASan+UBSan)" if sanitize else "", len(srcs)), flush=True)
    _run([cxx] + flags + ["-o", target] + srcs + ["-lpthread"])
    man = _load_manifest()
    man[section] = {"key": key, "source_digest": digest, "api": api_signatures("host"), "compiled": True,
                    "flags": flags, "time": time.strftime("%Y-%m-%dT%H:%M:%S")}
    _save_manifest(man)
    return target


def build_all(force: bool = False, jobs: int = 8, verbose: bool = False):
    k = build_kernels(force=force, jobs=jobs, verbose=verbose)
    h = build_host(force=force, verbose=verbose)
    return k, h


def check_fresh(which: str):
    """Raises if the library ``which`` ("kernels" / "host") was built from other sources than the
    tree holds (sources present but digest differs), i.e. a stale prebuilt binary. Returns the
    accepted manifest record's table of entry points (api_signatures at build time), or None when
    there is no such record."""
    srcs, _ = kernel_sources() if which == "kernels" else host_sources()
    if not srcs or os.environ.get("FMLX_SKIP_FRESHNESS", "0") == "1":
        return None
    rec = _load_manifest().get(which, {})
    if not rec:
        return None  # library built by hand / older tree: nothing to compare against
    if rec.get("source_digest") != source_digest(which):
        raise RuntimeError("native %s library is stale: built from other sources than this tree "
                           "(run python -m flink_ml_amd.ops.build)" % which)
    return rec.get("api")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--sanitize", action="store_true", help="also build the ASan/UBSan host runtime")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args(argv)
    k, h = build_all(force=a.force, jobs=a.j, verbose=True)
    print("built:", k, h)
    if a.sanitize:
        print("built:", build_host(force=a.force, verbose=True, sanitize=True))


if __name__ == "__main__":
    sys.exit(main())
