"""The stratified systems (tests/stratified_systems.py) under the oracle alone, no GPU: the
committed seed list meets the conditions that keep tests/test_gpu_stratified.py from passing
vacuously -- every system is served by the instance it is named after, rays get through, rays are
lost in the rear half, and with the apertures unchecked nearly all traverse every surface while
some still end in total reflection and some miss a surface.  Prints the table per system."""
import numpy as np
import pytest

from rayoptics_amd import abi

import stratified_systems as S


def shares(c):
    """the figures of one system, from the oracle's FULL traces of the ray list and the grid"""
    ref = S.oracle_results(c)
    N = c.table.n_ifcs
    out = {}
    for entry, key in (('list', 'list/%d/%d'), ('grid', f'grid/{c.wvl}/%d/%d')):
        chk, unc = ref[key % (abi.OUT_FULL, 1)], ref[key % (abi.OUT_FULL, 0)]
        failed = chk['status'] != abi.OK
        out[entry] = dict(ok=float((~failed).mean()),
                          late=float((failed & (chk['fail_surf'] >= N / 2)).mean()),
                          ok_unchecked=float((unc['status'] == abi.OK).mean()),
                          tir=int((unc['status'] == abi.TIR).sum()),
                          missed=int((unc['status'] == abi.MISSED_SURFACE).sum()))
    return out


@pytest.fixture(scope='module')
def table():
    rows = {c.name: shares(c) for c in S.cases()}
    print('\nsystem     N  mirror | list: ok  late  ok(unchecked) TIR MISSED | grid: ok  late  ok(unchecked)')
    for c in S.cases():
        l, g = rows[c.name]['list'], rows[c.name]['grid']
        print(f'{c.name:9s} {c.table.n_ifcs:2d}  {c.table.design["mirror"]:4d}   |     {l["ok"]:.3f} {l["late"]:.3f} '
              f'{l["ok_unchecked"]:.3f}      {l["tir"]:4d} {l["missed"]:4d}   |     {g["ok"]:.3f} {g["late"]:.3f} '
              f'{g["ok_unchecked"]:.3f}')
    return rows


@pytest.mark.parametrize('instance', S.INSTANCES)
def test_the_mirror_names_the_intended_instance(instance):
    for c in S.cases(instance):
        assert S.features(c.table) == S.SYSTEM_FEAT[instance], c.name
        assert S.INSTANCES[S.expected_instance(c.table, 0)] == instance, c.name
        # ROX_FILTER_PHANTOMS moves a system with a PHANTOM row to `general`, and no other
        want = 'general' if c.has_phantom else instance
        assert S.INSTANCES[S.expected_instance(c.table, abi.FILTER_PHANTOMS)] == want, c.name
    assert S.case(instance, 0).has_phantom and not S.case(instance, 1).has_phantom
    assert len(set(S.SEEDS[instance])) == 3


def test_every_system_carries_the_common_features():
    n_mirror = 0
    for c in S.cases():
        rows, N = c.table.rows, c.table.n_ifcs
        assert 10 <= N <= 14, c.name
        ident = np.eye(3).ravel().tolist()
        tilted = [r for r in rows if list(r.rt) != ident]
        assert sorted(r.rt_order for r in tilted) == [abi.RT_F_ORDER, abi.RT_C_ORDER], c.name
        assert all(r.t[0] != 0.0 and r.t[1] != 0.0 for r in tilted), c.name
        assert any(r.profile == abi.CONIC for r in rows), c.name
        assert sum(r.mode in (abi.DUMMY, abi.PHANTOM) for r in rows[1:N - 1]) == 1, c.name
        mirrors = [i for i in range(N) if rows[i].mode == abi.REFLECT]
        assert len(mirrors) <= 1
        n_mirror += len(mirrors)
        if mirrors:     # z_dir and the thickness signs flip behind the mirror
            m = mirrors[0]
            assert all(rows[i].z_dir == (1.0 if i < m else -1.0) for i in range(N)), c.name
            assert all((rows[i].t[2] > 0) == (i < m) for i in range(N - 1)), c.name
    assert 7 <= n_mirror <= 14, n_mirror      # about half of the 21 systems
    for instance in S.INSTANCES:            # per instance: one with and one without
        assert len({c.table.design['mirror'] > 0 for c in S.cases(instance)}) == 2, instance


def test_rays_get_through_every_system(table):
    for name, row in table.items():
        for entry in ('list', 'grid'):
            assert 0.20 <= row[entry]['ok'] <= 0.90, (name, entry, row[entry])


@pytest.mark.parametrize('instance', S.INSTANCES)
def test_rays_are_lost_in_the_rear_half(table, instance):
    for entry in ('list', 'grid'):
        assert max(table[c.name][entry]['late'] for c in S.cases(instance)) >= 0.01, (instance, entry)


@pytest.mark.parametrize('instance', S.INSTANCES)
def test_unchecked_rays_traverse_every_surface(table, instance):
    rows = [table[c.name] for c in S.cases(instance)]
    for entry in ('list', 'grid'):
        assert np.mean([r[entry]['ok_unchecked'] for r in rows]) >= 0.95, (instance, entry)
    assert sum(r['list']['tir'] for r in rows) >= 1, instance
    assert sum(r['list']['missed'] for r in rows) >= 1, instance
