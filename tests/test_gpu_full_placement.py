"""-m gpu: where a FULL launch puts its tiles and rows changes no bit of what it writes.

Every workgroup -> tile map (ROX_FULL_TILE_GROUP = 0, 4, 32; the variable is read once, so each
setting runs in a fresh child process, tests/full_placement_child.py) traces the double Gauss into
FULL packets -- a ragged 45 x 46 grid, 364 x 364 rays (130 tiles of 1024: one whole block of
8 x 16 and a remainder), a row block of it, two items through rox_trace_pupil_grids -- with the
1024-thread kernels (ROX_SMALL_BLOCKS=0), with the launch rule's own choice (256-thread workgroups
at these sizes) and through the chunk loop (ROX_RAYS_PER_LAUNCH=4096).  Each case is traced at
ld = rox_packet_ld(R), R and R + 1 over buffers whose row pads hold a sentinel: packets, op,
status, fail_surf and pupil equal the oracle's bit for bit, and no byte of a pad is written."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


@pytest.fixture(scope='module')
def oracle_refs(tmp_path_factory):
    """the oracle's result of every case, computed once, as <case>_<item>.npz"""
    from oracle import oracle
    import full_placement_child as child
    wl, flags = child.setup()
    d = tmp_path_factory.mktemp('full_placement')
    for name in child.CASES:
        flds, grid, opts = child.case_args(wl, flags, name, oracle.make_grid, oracle.make_opts)
        for i, fld in enumerate(flds):
            r = oracle.trace_pupil_grid(wl.table, fld, grid, child.WVL, opts)
            np.savez(os.path.join(d, f'{name}_{i}.npz'), seg=r.seg, op=r.op, status=r.status,
                     fail_surf=r.fail_surf, pupil=r.pupil)
    return str(d)


BIG = {'ROX_SMALL_BLOCKS': '0'}
CHUNKED = {'ROX_RAYS_PER_LAUNCH': '4096'}
SETTINGS = [(g, env) for g in (0, 4, 32) for env in (BIG, CHUNKED)] + \
    [(4, {}), (1, CHUNKED)]     # the launch rule's small workgroups; 16-tile launches that map


@pytest.mark.parametrize('group,extra', SETTINGS,
                         ids=[f'G{g}-' + ('-'.join(f'{k[4:].lower()}{v}' for k, v in e.items()) or 'default')
                              for g, e in SETTINGS])
def test_full_packets_do_not_depend_on_placement(oracle_refs, group, extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ('ROX_FULL_TILE_GROUP', 'ROX_SMALL_BLOCKS', 'ROX_RAYS_PER_LAUNCH')}
    env.update(extra, ROX_FULL_TILE_GROUP=str(group))
    p = subprocess.run([sys.executable, os.path.join(HERE, 'full_placement_child.py'), oracle_refs],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    failures = json.loads(p.stdout.strip().splitlines()[-1])['failures']
    assert not failures, failures
