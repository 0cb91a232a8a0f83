"""The kernel headers of ray-optics_amd/csrc are split by concern and the split is real: every
header compiles on its own, the host-only units see no kernel code, and rox_device.hpp is
nothing but the list of its pieces.  Needs hipcc, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ray-optics_amd', 'csrc')
HIPCC = next((c for c in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc')
              if c and os.path.exists(c)), None)
pytestmark = pytest.mark.skipif(HIPCC is None, reason='hipcc not found')

FRONT = ['-x', 'hip', '--offload-arch=gfx950', '-std=c++17', '-Wno-pragma-once-outside-header']
PIECES = ['rox_config.hpp', 'rox_args.hpp', 'rox_math.hpp', 'rox_math_fast.hpp', 'rox_profiles.hpp',
          'rox_phase.hpp', 'rox_opd.hpp', 'rox_ray.hpp', 'rox_compact.hpp', 'rox_kernel.hpp']
HOST_UNITS = ['launch.hip', 'trace_entries.hip', 'search_entries.hip', 'roxtrace.hip', 'focus.hip']
KERNEL_CODE = ['rox_kernel.hpp', 'rox_ray.hpp']


def umbrella_includes():
    with open(os.path.join(CSRC, 'rox_device.hpp')) as f:
        return re.findall(r'^#include "([^"]+)"', f.read(), re.M)


def test_the_umbrella_lists_every_piece():
    assert umbrella_includes() == PIECES
    assert all(os.path.exists(os.path.join(CSRC, h)) for h in PIECES)


@pytest.mark.parametrize('header', PIECES + ['rox_device.hpp'])
def test_header_compiles_on_its_own(header):
    r = subprocess.run([HIPCC, *FRONT, '-fsyntax-only', os.path.join(CSRC, header)],
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize('unit', HOST_UNITS)
def test_host_unit_sees_no_kernel_code(unit):
    for side in ('--cuda-host-only', '--cuda-device-only'):
        r = subprocess.run([HIPCC, *FRONT, side, '-E', os.path.join(CSRC, unit), '-o', '-'],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        seen = {os.path.basename(m) for m in re.findall(r'^# \d+ "([^"]+)"', r.stdout, re.M)}
        assert 'rox_args.hpp' in seen and 'rox_config.hpp' in seen      # (the markers are being read)
        assert not seen & set(KERNEL_CODE), (side, sorted(seen & set(KERNEL_CODE)))


def test_the_umbrella_is_includes_and_comments():
    with open(os.path.join(CSRC, 'rox_device.hpp')) as f:
        code = [ln.split('//')[0].strip() for ln in f]
    rest = [ln for ln in code if ln and ln != '#pragma once' and not re.fullmatch(r'#include "rox_\w+\.hpp"', ln)]
    assert rest == []
