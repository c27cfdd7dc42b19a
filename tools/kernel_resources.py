"""registers / scratch / spills / instruction count / code digest of every kernel of one csrc/*.hip file (cross-compiles, no GPU):
python tools/kernel_resources.py rollout_chain.hip [-D...]
The compile and the parser are the test suite's (tests/build_common.py), so the figures are the ones the ISA tests pin.  The digest is the SHA-1 of a kernel's
instruction lines without their place in the file: run this at two commits and diff the output to see which kernels a change of the sources touched."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from build_common import device_asm  # noqa: E402

asm = device_asm(sys.argv[1], sys.argv[2:])
for name in asm.kernel_names():
    k = asm.kernel(name)
    r = k.resources
    print("%-76s agpr %3d vgpr %3d scratch %4d sgpr_spill %3d vgpr_spill %3d instructions %5d digest %s"
          % (name, r["agpr"], r["vgpr"], r["scratch"], r["sgpr_spill"], r["vgpr_spill"], len(k.body), k.digest()))
