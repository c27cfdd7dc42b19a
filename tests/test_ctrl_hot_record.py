"""The launch-invariant data the rollout step reads without going back to global memory for descriptors (CPU suite):

  * the chain kernel's ISA holds no flat_load / flat_store in any instantiation -- every table a step reads is typed as global memory, so its loads are
    global_load (counted by vmcnt alone) -- and the chains of the forest come out of a register (v_readlane), not out of MechDev, in the Newton loop;
  * the controller's hot record (CtrlDev::hot, csrc/cclqr_dev.h ctrl_hot_build) equals the CtrlDev fields it copies, field for field: one shared
    table and one per instance (n_ctrl > 1), finite and infinite horizon, with and without gains / feed-forward / friction / noise / PID;
  * the row addresses a step forms from the record alone (ctrl_step_rows) are the addresses of the CtrlDev indexing the kernels used before
    (tests/emu/emu_ctrl_hot.cpp keeps that indexing), on the hanging 17-body chain, a forest of two chains and the tracking law;
  * the chain plan word decodes to MechDev's chains."""
import ctypes as C

import numpy as np
import pytest

from build_common import device_asm, host_library
from conftest import hanging_setpoint, long_and_short_chain_forest

FIELDS = ["mu", "nK", "N", "nsp", "K", "zd", "Fd", "K_stride", "zd_stride", "Fd_stride", "has_fric", "has_pid", "noise_on", "noise_scale", "noise_key0"]


@pytest.fixture(scope="module")
def hot():
    lib = host_library("libemu_hot.so", ["emu/emu_ctrl_hot.cpp"])
    lib.emu_ctrl_hot_rows.restype = C.c_longlong
    return lib


def controllers(cclqr):
    """(name, tables, ctrl_desc keyword arguments, lanes of the instance's group)"""
    rng = np.random.default_rng(21)
    out = []
    t17 = cclqr.examples.cartpole_n(16)["mech"].tables()
    zd17 = hanging_setpoint(cclqr, 16)
    out.append(("hanging 17-body chain, finite horizon", t17, dict(ctrl_joint=[0], K=rng.normal(size=(29, 1, 12 * t17.nb)), N=30, zd=zd17), 32))
    out.append(("hanging 17-body chain, infinite horizon", t17, dict(ctrl_joint=[0], K=rng.normal(size=(1, 1, 12 * t17.nb)), N=0, zd=zd17), 32))
    nc = 5
    out.append(("17-body chain, a table per instance, infinite horizon", t17,
                dict(ctrl_joint=[0], K=rng.normal(size=(nc, 1, 1, 12 * t17.nb)), N=0, zd=np.repeat(zd17[None, None], nc, 0), Fd=rng.normal(size=(nc, 1, 1)), n_ctrl=nc), 32))
    out.append(("17-body chain, a table per instance, finite horizon", t17,
                dict(ctrl_joint=[0], K=rng.normal(size=(nc, 9, 1, 12 * t17.nb)), N=10, zd=np.repeat(zd17[None, None], nc, 0), n_ctrl=nc), 32))
    tf, _, zdf, Kf, cjf = long_and_short_chain_forest(cclqr)
    out.append(("forest of two chains, two inputs", tf, dict(ctrl_joint=list(cjf), K=Kf, N=Kf.shape[0] + 1, zd=zdf), 32))
    t4 = cclqr.examples.triple_cartpole()["mech"].tables()
    T = 40      # tracking: a setpoint, a feed-forward row and a gain table per step, friction, Philox noise
    zd4 = np.zeros((T, t4.nb, 13)); zd4[:, :, 3] = 1.0; zd4[:, :, 0:3] = rng.normal(size=(T, t4.nb, 3))
    out.append(("tracking law on the triple cartpole", t4, dict(ctrl_joint=[0], K=rng.normal(size=(T - 1, 1, 12 * t4.nb)), N=T, zd=zd4, Fd=rng.normal(size=(T, 1)),
                                                                fric=[0.1] * t4.nb, noise_scale=2.0, noise_seed=0xC0FFEE), 8))
    out.append(("feed-forward only + PID", t4, dict(ctrl_joint=[0, 1], N=0, zd=zd4[0], Fd=rng.normal(size=(1, 2)),
                                                    pid=dict(joint=[2], P=[1.0], I=[0.1], D=[0.01], goal=[0.3])), 8))
    return out


def test_hot_record_matches_ctrl_tables_field_for_field(cclqr, orc, hot):
    for name, t, kw, _ in controllers(cclqr):
        m, c = orc.mech_desc(t), orc.ctrl_desc(t.nb, **kw)
        dev, rec = np.zeros(96, dtype=np.int64), np.zeros(96, dtype=np.int64)
        n = hot.emu_ctrl_hot_fields(C.byref(m.desc), C.byref(c.desc), dev.ctypes.data_as(C.POINTER(C.c_longlong)), rec.ctypes.data_as(C.POINTER(C.c_longlong)), 96)
        mu = len(kw["ctrl_joint"])
        assert n == len(FIELDS) + mu, (name, n)
        names = FIELDS + ["cj[%d]" % i for i in range(mu)]
        for i in range(n):
            assert dev[i] == rec[i], "%s: CtrlDev.%s = %d, record holds %d" % (name, names[i], dev[i], rec[i])
        got = dict(zip(names, dev[:n]))
        assert got["mu"] == mu and got["N"] == kw["N"] and got["zd"] != 0 and (got["K"] != 0) == ("K" in kw)
        assert (got["K_stride"] != 0) == (kw.get("n_ctrl", 0) > 1 and "K" in kw) and (got["zd_stride"] != 0) == (kw.get("n_ctrl", 0) > 1)
        assert got["has_fric"] == ("fric" in kw) and got["has_pid"] == ("pid" in kw) and got["noise_on"] == ("noise_scale" in kw)


def test_rows_from_the_record_are_the_rows_of_the_table_indexing(cclqr, orc, hot):
    for name, t, kw, G in controllers(cclqr):
        m, c = orc.mech_desc(t), orc.ctrl_desc(t.nb, **kw)
        n_inst = max(kw.get("n_ctrl", 0), 3)
        checked = C.c_longlong(0)
        # steps on both sides of the horizon N and of the last setpoint / gain table; instances from a global index > 0 (a shard of a batch)
        for inst0, n in ((0, n_inst), (2, n_inst - 2)):
            bad = hot.emu_ctrl_hot_rows(C.byref(m.desc), C.byref(c.desc), C.c_longlong(inst0), C.c_longlong(n), 1, 60, G, C.byref(checked))
            assert bad == 0, "%s: %d of %d addresses differ" % (name, bad, checked.value)
            assert checked.value >= 60 * n * (3 + t.nb)


def test_chain_plan_word_decodes_to_the_chains(cclqr, orc, hot):
    forest = long_and_short_chain_forest(cclqr)[0]
    for t, nchains in ((cclqr.examples.cartpole_n(16)["mech"].tables(), 1), (forest, 2), (cclqr.examples.cartpole_n(1)["mech"].tables(), 1)):
        m = orc.mech_desc(t)
        words, n = np.zeros(64, dtype=np.int32), C.c_int(0)
        bad = hot.emu_chain_plan(C.byref(m.desc), words.ctypes.data_as(C.POINTER(C.c_int)), C.byref(n))
        assert bad == 0 and n.value == nchains
        lens = [(int(w) >> 8) & 0xff for w in words[:nchains]]
        assert sum(lens) == t.nb and all(((int(w) >> 8) & 0xffff) == nchains << 8 for w in words[nchains:])      # lanes past the last chain: length 0


def test_chain_kernels_read_their_tables_through_global_loads():
    """every rollout_chain_kernel instantiation: no flat memory instruction (the address space of every table is visible to the compiler), the chains
    come out of the plan register, and the controller's record comes through scalar loads"""
    asm = device_asm("rollout_chain.hip")
    starts = asm.kernel_names("_ZN5cclqr20rollout_chain_kernelI")
    assert len(starts) == 35, len(starts)
    for name in starts:
        ops = asm.kernel(name).ops
        flat = [o for o in ops if o.startswith(("flat_load", "flat_store", "flat_atomic"))]
        assert not flat, (name, flat[:4])
        assert any(o.startswith("v_readlane_b32") for o in ops), name                       # the chain plan
        assert sum(o.startswith("s_load_dwordx8") or o.startswith("s_load_dwordx16") for o in ops) >= 1, name      # the record, one wide scalar load
        assert sum(o.startswith("global_load") for o in ops) > 0 and sum(o.startswith("global_store") for o in ops) > 0, name
