"""tests/build_common.py, the suite's one build helper (CPU suite): the parser on an assembly text written out here, the one-compile-per-source cache on the
smallest kernel source, and the rule that rebuilds a host library on a toy source and header.  The parser's test on real kernels are the 25 digests and the
instruction counts of tests/test_chain_*_isa.py."""
import os

import build_common as bc

FOO, BAR = "_ZN5cclqr3fooEv", "_ZN5cclqr3barEv"


def _function(name, number, sep, operand):
    """one kernel the way the compiler writes it: directives, the label with its comment, block labels numbered by function, comments, a resource block"""
    return """\t.protected\t%(name)s ; -- Begin function %(name)s
\t.globl\t%(name)s
\t.p2align\t8
\t.type\t%(name)s,@function
%(name)s: ; @%(name)s
; %%bb.0:
\ts_load_dwordx2%(sep)ss[0:1], s[0:1], 0x0
\tv_mov_b32_e32%(sep)sv1, %(operand)s

\ts_cbranch_vccnz%(sep)s.LBB%(number)d_7
; %%bb.1:
\tv_add_f64%(sep)sv[2:3], v[2:3], v[4:5]    ; a trailing comment stays with its line
toy_label:
.LBB%(number)d_7:                                ; =>This Inner Loop Header: Depth=1
\tglobal_store_dword%(sep)sv0, v1, s[0:1]
.Ltmp%(number)d:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel %(name)s
\t\t.amdhsa_next_free_vgpr 6
\t.end_amdhsa_kernel
.Lfunc_end%(number)d:
\t.set %(name)s.num_vgpr, 6
; Kernel info:
; TotalNumVgprs: %(total)d
; ScratchSize: %(scratch)d
""" % dict(name=name, number=number, sep=sep, operand=operand, total=6 + number, scratch=16 * number)


METADATA = """\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     2
    .args:
      - .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .group_segment_fixed_size: 64
    .name:           %s
    .private_segment_fixed_size: 48
    .sgpr_count:     12
    .sgpr_spill_count: 3
    .symbol:         %s.kd
    .vgpr_count:     9
    .vgpr_spill_count: 1
  - .agpr_count:     0
    .args:           []
    .group_segment_fixed_size: 0
    .name:           %s
    .private_segment_fixed_size: 0
    .sgpr_count:     10
    .sgpr_spill_count: 0
    .vgpr_count:     6
    .vgpr_spill_count: 0
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
...
\t.end_amdgpu_metadata
""" % (FOO, FOO, BAR)


def _asm(foo=(3, "\t", "0"), bar=(4, "   ", "0")):
    return bc.parse_asm("\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n" + _function(FOO, *foo) + _function(BAR, *bar) + METADATA)


def test_parser_reads_what_the_text_says():
    asm = _asm()
    assert isinstance(asm.lines, tuple)
    assert asm.kernel_names() == [FOO, BAR] and asm.kernel_names("_ZN5cclqr3b") == [BAR]
    foo, bar = asm.kernel(FOO), asm.kernel(BAR)
    # the label line carries a comment, so it does not end in ":" and counts as a line of the body: that is the rule every pinned count was taken with
    assert foo.body == (FOO + ": ; @" + FOO, "s_load_dwordx2\ts[0:1], s[0:1], 0x0", "v_mov_b32_e32\tv1, 0", "s_cbranch_vccnz\t.LBB3_7",
                        "v_add_f64\tv[2:3], v[2:3], v[4:5]    ; a trailing comment stays with its line", "global_store_dword\tv0, v1, s[0:1]")
    assert foo.ops == (FOO + ":", "s_load_dwordx2", "v_mov_b32_e32", "s_cbranch_vccnz", "v_add_f64", "global_store_dword")
    assert bar.ops[1:] == foo.ops[1:] and bar.body[3] == "s_cbranch_vccnz   .LBB4_7"
    # raw: the same range untouched, from the label to the line in front of s_endpgm
    assert foo.raw[0] == FOO + ": ; @" + FOO and foo.raw[-1] == ".Ltmp3:" and "" in foo.raw and len(foo.raw) == 12 and "toy_label:" in foo.raw
    assert [l for l in foo.raw if "v_mov" in l] == ["\tv_mov_b32_e32\tv1, 0"]
    # tail: from s_endpgm to the next kernel's label, no further
    assert foo.tail[0] == "\ts_endpgm" and "; TotalNumVgprs: 9" in foo.tail and "; ScratchSize: 48" in foo.tail
    assert not [l for l in foo.tail if "TotalNumVgprs: 10" in l] and foo.tail[-1] == "\t.type\t%s,@function" % BAR
    assert "; TotalNumVgprs: 10" in bar.tail and "; ScratchSize: 64" in bar.tail
    assert dict(foo.resources) == dict(agpr=2, vgpr=9, scratch=48, lds=64, sgpr_spill=3, vgpr_spill=1)
    assert dict(bar.resources) == dict(agpr=0, vgpr=6, scratch=0, lds=0, sgpr_spill=0, vgpr_spill=0)
    assert asm.kernel(FOO) is foo


def test_digest_ignores_blanks_and_the_function_number_only():
    a = _asm(foo=(3, "\t", "0"), bar=(4, "   ", "0"))
    # the two kernels differ in their name line, so compare each with itself across two files: other blanks, other function number
    b = _asm(foo=(5, "  \t ", "0"), bar=(9, " ", "0"))
    assert a.kernel(FOO).body != b.kernel(FOO).body
    assert a.kernel(FOO).digest() == b.kernel(FOO).digest() and a.kernel(BAR).digest() == b.kernel(BAR).digest()
    assert len(a.kernel(FOO).digest()) == 16 and a.kernel(FOO).digest() != a.kernel(BAR).digest()
    c = _asm(foo=(3, "\t", "1"))
    assert c.kernel(FOO).digest() != a.kernel(FOO).digest() and c.kernel(BAR).digest() == a.kernel(BAR).digest()


def test_a_source_is_compiled_once_per_process():
    n = len(bc.device_compiles)
    first = bc.device_asm("score.hip")
    assert len(bc.device_compiles) == n + 1 and bc.device_compiles[-1][:2] == ("score.hip", ())      # no other test of the suite compiles score.hip
    assert bc.device_asm("score.hip") is first and len(bc.device_compiles) == n + 1
    assert first.kernel_names() and all(first.kernel(k).ops[-1] != "s_endpgm" and first.kernel(k).resources["vgpr"] > 0 for k in first.kernel_names())
    assert bc.device_asm("score.hip", ("-DCCLQR_TEST_BUILD_COMMON",)) is not first and len(bc.device_compiles) == n + 2      # other flags, another entry


def test_a_library_older_than_anything_it_includes_is_rebuilt(tmp_path):
    inc, out = tmp_path / "inc", tmp_path / "out"
    inc.mkdir(), out.mkdir()
    header, source = inc / "toy.h", tmp_path / "toy.c"
    header.write_text("#define TOY 41\n")
    source.write_text('#include "inc/toy.h"\nint toy(void) { return TOY + 1; }\n')
    build = lambda: bc.host_library("libtoy.so", [str(source)], compiler="cc", flags=("-shared", "-fPIC"), watched=(str(inc),), out_dir=str(out))
    so = str(out / "libtoy.so")
    n = len(bc.host_builds)
    assert build().toy() == 42 and len(bc.host_builds) == n + 1 and bc.host_builds[-1][0] == so
    built = os.stat(so).st_mtime_ns
    assert build().toy() == 42 and len(bc.host_builds) == n + 1 and os.stat(so).st_mtime_ns == built
    later = built + 5 * 10 ** 9
    os.utime(header, ns=(later, later))
    build()
    assert len(bc.host_builds) == n + 2 and os.stat(so).st_mtime_ns != built
    assert sorted(os.listdir(out)) == ["libtoy.so"]
