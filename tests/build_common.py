"""The test suite's one build helper: what the tests compile besides the product itself, and how they read it.

  * device_asm(src_name) cross-compiles one csrc/*.hip file to gfx950 assembly with the flags every ISA pin of this repository was measured with, ONCE per
    process: the tests/test_chain_*_isa.py files, the resource tests of test_host.py, test_ctrl_hot_record.py and tools/kernel_resources.py all read the same
    parsed object.  There is no cache on disk, so a pin can never be checked against the assembly of an earlier source.
  * Asm.kernel(name) is the one parser from a mangled kernel name to its instruction lines, its resource comments and its metadata, and
    Kernel.digest() the one normalisation under which two builds of a kernel are "the same device code".
  * host_library(so_name, sources) builds a CPU twin (tests/emu/*.cpp) or a small GPU helper (tests/gpu/*.hip) into tests/emu/ and loads it.  It rebuilds
    when the library is older than ANY file it could have been built from -- its sources, everything under csrc/, include/cclqr.h, every tests/emu/*.cpp
    -- instead of a list of headers kept by hand next to each call: a twin built from an older header made the bit-for-bit comparisons against it pass for
    the wrong reason.

The `emu` fixture of tests/conftest.py keeps its own compile line and its own list of headers: it is the one copy left outside this module.  conftest.py is
part of how every change to this repository is tested, so a change to the tests' helpers does not edit it."""
import ctypes
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile
import time
from dataclasses import dataclass
from functools import lru_cache
from types import MappingProxyType

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CSRC = os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc")
EMU = os.path.join(TESTS, "emu")
HIPCC = "/opt/rocm/bin/hipcc"
# every pinned count and digest was measured with these flags
DEVICE_FLAGS = ("-O3", "-std=c++17", "-ffp-contract=fast", "--offload-arch=gfx950", "-S", "--cuda-device-only")
# the bit-equality tests against the twins rest on -ffp-contract=off
HOST_FLAGS = ("-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-shared")
# what a library under tests/emu/ can have been built from: a directory stands for every file under it but the objects `make` leaves there, anything
# else is a glob pattern
WATCHED = (CSRC, os.path.join(ROOT, "include", "cclqr.h"), os.path.join(EMU, "*.cpp"))
OBJECTS = (".o", ".a", ".so")

KERNEL = "_ZN5cclqr20rollout_chain_kernelILi%dELi%dELi%dELb%dELi%dELi%dEEEvNS_11RolloutArgsE"


def chain_kernel(G, NBP, EXTRA, RELAX, KL, NL):
    """mangled name of rollout_chain_kernel<G, NBP, EXTRA, RELAX, KL, NL> (csrc/rollout_chain.hip)"""
    return KERNEL % (G, NBP, EXTRA, RELAX, KL, NL)


HEADLINE = chain_kernel(32, 17, 0, False, 1, 32)

device_compiles = []        # (src_name, extra_flags, seconds) of every real compile of this process, in order: its length is the counter
host_builds = []            # (path of the library, seconds) of every real build of this process
_asm = {}


def _run(cmd):
    t0 = time.time()
    p = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if p.returncode:
        raise RuntimeError("%s\nexit status %d\n%s" % (" ".join(cmd), p.returncode, p.stderr[-4000:]))
    return time.time() - t0


@dataclass(frozen=True)
class Kernel:
    name: str
    raw: tuple          # the lines from `name:` up to the first s_endpgm, as the compiler wrote them
    body: tuple         # the same range stripped, without blank lines, comment lines, directives and labels
    ops: tuple          # first word of each body line
    tail: tuple         # from that s_endpgm to the next cclqr symbol: the "; Kernel info:" comments (TotalNumVgprs, ScratchSize, ...)
    resources: object   # agpr, vgpr, scratch, lds, sgpr_spill, vgpr_spill of the kernel's metadata entry (None for a function that is no kernel)

    def normalised(self):
        """the body with blanks squeezed and the function number taken out of the branch labels: equal for two builds of a kernel that differ in nothing
        but their place in the file"""
        return "\n".join(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", l)) for l in self.body)

    def digest(self):
        """first 16 hex digits of the SHA-1 of normalised()"""
        return hashlib.sha1(self.normalised().encode()).hexdigest()[:16]


@dataclass(frozen=True, eq=False)
class Asm:
    lines: tuple
    _labels: object     # symbol -> index of its label line
    _resources: object  # kernel name -> resources, in the order of the metadata

    def kernel_names(self, prefix=""):
        """the kernels of the file (entries of its amdhsa.kernels metadata) whose mangled name starts with prefix, in file order"""
        return [n for n in self._resources if n.startswith(prefix)]

    @lru_cache(maxsize=None)
    def kernel(self, name):
        lines = self.lines
        start = self._labels[name]
        end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
        body = tuple(l for l in (x.strip() for x in lines[start:end]) if l and not l.startswith((";", ".")) and not l.endswith(":"))
        tail = []
        for l in lines[end:]:
            if l.startswith("_ZN5cclqr"):
                break
            tail.append(l)
        return Kernel(name, lines[start:end], body, tuple(l.split()[0] for l in body), tuple(tail), self._resources.get(name))


def parse_asm(text):
    """Asm of the text of one gfx950 assembly file"""
    lines = tuple(text.splitlines())
    labels = {}
    for i, l in enumerate(lines):
        m = re.match(r"([A-Za-z_$][\w$.]*):", l)
        if m:
            labels.setdefault(m.group(1), i)
    resources = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
        resources[re.search(r"\.name:\s+(\S+)", blk).group(1)] = MappingProxyType(dict(
            agpr=int(blk.split()[0]), vgpr=g("vgpr_count"), scratch=g("private_segment_fixed_size"), lds=g("group_segment_fixed_size"),
            sgpr_spill=g("sgpr_spill_count"), vgpr_spill=g("vgpr_spill_count")))
    return Asm(lines, MappingProxyType(labels), MappingProxyType(resources))


def device_asm(src_name, extra_flags=()):
    """csrc/<src_name> cross-compiled for gfx950 and parsed; compiled once per process and (src_name, extra_flags)"""
    key = (src_name, tuple(extra_flags))
    if key not in _asm:
        with tempfile.TemporaryDirectory(prefix="cclqr_isa_") as d:
            asm = os.path.join(d, src_name + ".s")
            dt = _run([HIPCC, *DEVICE_FLAGS, "-o", asm, os.path.join(CSRC, src_name), *key[1]])
            text = open(asm).read()
        device_compiles.append(key + (dt,))
        print("build_common: device compile %s %s%.0f s" % (src_name, "".join(f + " " for f in key[1]), dt), file=sys.stderr, flush=True)
        _asm[key] = parse_asm(text)
    return _asm[key]


def _newest(watched):
    files = []
    for w in watched:
        if os.path.isdir(w):
            files += [os.path.join(d, f) for d, _, fs in os.walk(w) for f in fs if not f.endswith(OBJECTS)]
        else:
            files += glob.glob(w)
    return max(os.path.getmtime(f) for f in files)


def host_library(so_name, sources, compiler=HIPCC, flags=HOST_FLAGS, watched=WATCHED, out_dir=EMU):
    """ctypes.CDLL of <out_dir>/<so_name>, built from `sources` (paths relative to tests/) when it is missing or older than the newest of its sources
    and of everything `watched` names.  argtypes / restype are the caller's business."""
    so = os.path.join(out_dir, so_name)
    srcs = [os.path.join(TESTS, s) for s in sources]
    if not os.path.exists(so) or os.path.getmtime(so) < _newest(list(watched) + srcs):
        tmp = "%s.%d.tmp" % (so, os.getpid())       # an interrupted build, or two processes building at once, never leave a partial file with a fresh date
        try:
            dt = _run([compiler, *flags, "-o", tmp, *srcs])
            os.replace(tmp, so)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        host_builds.append((so, dt))
        print("build_common: host build %s %.0f s" % (so_name, dt), file=sys.stderr, flush=True)
    return ctypes.CDLL(so)
