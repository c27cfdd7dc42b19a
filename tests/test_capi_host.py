"""The host arithmetic of csrc/capi.hip that is stated once in csrc/cclqr_internal.h, on the CPU (tests/emu/emu_capi_host.cpp): the layout of a controller's
gain tables and the choice between the Riccati kernels that assume a symmetric Pk and those that do not."""
import ctypes as C

import numpy as np
import pytest

from capi_host_common import emu_capi_host


@pytest.fixture(scope="module")
def host():
    return emu_capi_host()


def _closed_form(G, NBP, nb):
    """doubles the control phase reads past a gain row: ceil(12 NBP / G) G - 12 nb, rounded up to even, 0 when not positive"""
    over = -(-12 * NBP // G) * G - 12 * nb
    return (over + 1) // 2 * 2 if over > 0 else 0


def _layout(host, loop, G, NBP, nb, n_tables, rows):
    out = (C.c_longlong * 4)()
    host.emu_gain_table_layout(loop, G, NBP, nb, n_tables, rows, out)
    return dict(zip(("pad", "stride", "K_stride", "alloc"), out))


def test_gain_row_overrun_is_the_closed_form(host):
    for G, NBP, nb, pad in ((8, 4, 2, 24), (8, 4, 3, 12), (8, 4, 4, 0), (16, 8, 5, 36), (32, 16, 9, 84), (32, 17, 17, 20), (64, 64, 33, 372)):      # worked by hand
        assert host.emu_gain_row_overrun(0, G, NBP, nb) == pad == _closed_form(G, NBP, nb)
        assert host.emu_gain_row_overrun(1, G, NBP, nb) == 0                 # the closed-loop kernel reads the exact row length
    for G in (8, 16, 32, 64):
        for NBP in range(1, 65):
            for nb in range(1, 65):                                          # (nb > NBP does not occur: the closed form still holds, 0 when not positive)
                assert host.emu_gain_row_overrun(0, G, NBP, nb) == _closed_form(G, NBP, nb)
    assert host.emu_gain_row_overrun(0, 32, 17, 19) == 0 and host.emu_gain_row_overrun(0, 16, 5, 1) == 52      # 12 x 5 = 60 -> 64 read, 12 kept
    # whatever image of at most 64 links a mechanism runs on, the overrun is at most 12 x 64 - 12 = 756 <= CCLQR_K_PAD
    assert max(_closed_form(G, NBP, nb) for G in (8, 16, 32, 64) for NBP in range(1, 65) for nb in range(1, 65)) == 756 <= host.emu_k_pad()


def test_gain_table_layout(host):
    K_PAD = host.emu_k_pad()
    assert K_PAD == 768
    for G, NBP, nb in ((8, 4, 2), (8, 4, 4), (16, 8, 5), (32, 17, 17), (64, 64, 33)):
        for rows in (1, 7, 199):
            for n in (0, 1):                                                 # one shared table: no pad, stride 0 in the controller's record
                L = _layout(host, 0, G, NBP, nb, n, rows)
                assert L == dict(pad=0, stride=rows * 12 * nb, K_stride=0, alloc=rows * 12 * nb + K_PAD)
            for n in (2, 64, 5000):                                          # one table per instance, each behind its own pad
                L = _layout(host, 0, G, NBP, nb, n, rows)
                pad = _closed_form(G, NBP, nb)
                assert L["pad"] == pad and L["stride"] == rows * 12 * nb + pad and L["K_stride"] == L["stride"] and L["alloc"] == n * L["stride"] + K_PAD
            L = _layout(host, 1, G, NBP, nb, 64, rows)                       # closed loops: tables back to back
            assert L["pad"] == 0 and L["K_stride"] == rows * 12 * nb and L["alloc"] == 64 * rows * 12 * nb + K_PAD
    big = _layout(host, 0, 64, 64, 64, 1 << 20, 999)                         # 6e11 doubles: no 32-bit intermediate
    assert big["alloc"] == (1 << 20) * 999 * 768 + K_PAD


def test_pad_of_every_launch_shape_fits_the_zero_tail(cclqr, orc, emu, host):
    """for every shape csrc/cclqr_tables.h rollout_shape_of returns -- chains of 1 .. 64 links, branching trees up to 64 links, a closed loop -- the per-table pad
    is at most CCLQR_K_PAD (worst case 12 x 64 - 12 = 756 <= 768): the read past the LAST table's last row stays inside the allocation"""
    from test_tree import _random_parents, build

    def shape(t):
        out = (C.c_longlong * 9)()
        assert emu.emu_rollout_shape(C.byref(orc.mech_desc(t).desc), out) == 0
        return out[0], out[1], out[2]

    mechs = [cclqr.examples.pendulum()["mech"].tables()] + [cclqr.examples.cartpole_n(nb - 1)["mech"].tables() for nb in range(2, 65)]
    mechs += [build(cclqr, "deep")["mech"].tables(), build(cclqr, "dual_cartpole")["mech"].tables(), cclqr.examples.deltabot()["mech"].tables()]
    for nb, seed in ((33, 1), (48, 3), (49, 4), (64, 5)):
        parents = _random_parents(np.random.default_rng(6000 + seed), nb)
        if not any(parents.count(a) > 1 for a in set(parents) if a >= 0):
            parents[-1] = parents[-2] if parents[-2] >= 0 else 0
        mechs.append(cclqr.examples.tree_mechanism(parents, seed=seed)["mech"].tables())
    worst, families = 0, set()
    for t in mechs:
        family, G, NBP = shape(t)
        families.add(family)
        pad = host.emu_gain_row_overrun(int(family == 2), G, NBP, t.nb)
        assert 0 <= pad <= host.emu_k_pad() and (family != 2 or pad == 0)
        worst = max(worst, pad)
    assert families == {0, 1, 2} and worst == 12 * 64 - 12 * 33             # the 33-link chain, the shortest on the 64-link image


def test_the_linearisation_kernel_stops_fitting_lds_at_57_links(cclqr, orc, emu):
    """csrc/cclqr_tables.h rollout_shape_of: one knot of a 56-link chain takes 163 080 of a compute unit's 163 840 bytes of LDS in the linearisation kernel, a
    57-link chain 165 992 -- the mechanism cclqr_mech_create accepts and the linearising entry points refuse (tests/test_gpu_setup.py)"""
    def lin_lds(n_links):
        out = (C.c_longlong * 9)()
        assert emu.emu_rollout_shape(C.byref(orc.mech_desc(cclqr.examples.cartpole_n(n_links)["mech"].tables()).desc), out) == 0
        return out[8], out[6]
    assert lin_lds(55) == (163080, 76808) and lin_lds(56) == (165992, 76808)
    assert lin_lds(55)[0] <= 160 * 1024 < lin_lds(56)[0] and lin_lds(56)[1] <= 160 * 1024      # (the rollout kernel takes both)


def test_ric_p_rows(host):
    rng = np.random.default_rng(0)
    mx, mu = 24, 3
    Q = rng.normal(size=(mx, mx)); Q = Q + Q.T
    R = rng.normal(size=(mu, mu)); R = R + R.T
    p = lambda A: A.ctypes.data_as(C.c_void_p)
    assert host.emu_ric_p_rows(p(Q), mx, p(R), mu) == 0
    Q1 = Q.copy(); Q1[3, 17] = np.nextafter(Q1[3, 17], np.inf)               # one off-diagonal entry one ulp apart from its mirror
    R1 = R.copy(); R1[2, 0] = np.nextafter(R1[2, 0], -np.inf)
    assert host.emu_ric_p_rows(p(Q1), mx, p(R), mu) == 1 and host.emu_ric_p_rows(p(Q), mx, p(R1), mu) == 1
    Qd = Q.copy(); Qd[5, 5] += 1.0                                           # the diagonal does not matter
    assert host.emu_ric_p_rows(p(Qd), mx, p(R), mu) == 0
    assert host.emu_ric_p_rows(p(Q), mx, None, 0) == 0 and host.emu_ric_p_rows(p(Q1), mx, None, 0) == 1      # mu = 0: R is not touched
