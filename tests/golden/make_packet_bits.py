"""Generates tests/golden/packet_bits.json: the SHA-256 digest of every output array of the calls
in tests/packet_bits_cases.py, by name.  Needs a GPU.

    python tests/golden/make_packet_bits.py

It is run at the commit whose bits are to be kept: the file committed was written by the library
before the packet entries came to share their tile walk, wave merge and launch turn, and
tests/test_gpu_packet_bits.py holds every later library to it.  The sums of these entries have a
fixed order, so the digests do not depend on the run."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', '..'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import packet_bits_cases as PB  # noqa: E402
from rayoptics_amd import abi  # noqa: E402


def main():
    eng, res, one, table = PB.make_world(torch)
    st = PB.statuses(res)
    assert all((s == abi.OK).any() for s in st), 'an item without OK rays'
    assert any((s != abi.OK).any() for s in st), 'no ray fails'
    print('rays OK per item', [int((s == abi.OK).sum()) for s in st], 'of', PB.NUM * PB.NUM,
          '; statuses', sorted(set(np.concatenate(st).tolist())))
    _window, box = PB.wide_window(eng, res)
    assert box > PB.LDS_BINS, f'the largest box of a tile, {box} bins, fits the LDS window'
    print('largest box of a tile at 80 x 80 bins:', box, 'bins')
    arrays = PB.run(eng, res, one, table)
    dig = PB.digests(arrays)
    for bins in (16, 80):
        for d in ('host', 'device'):
            for n in ('wmaps', 'counts', 'scale_exp', 'item'):
                got = {dig[f'weighted_maps/bins{bins}_path_{p or "default"}/{d}/{n}'] for p in PB.PATHS}
                assert len(got) == 1, f'the scatter paths differ: bins {bins} {d} {n}'
    assert arrays['weighted_maps/bins80_path_default/host/counts'].sum() > 0
    again = PB.digests(PB.run(eng, res, one, table))
    assert again == dig, 'a second run differs: ' + str([k for k in dig if dig[k] != again[k]])
    eng.close()
    path = os.path.join(HERE, 'packet_bits.json')
    with open(path, 'w') as f:
        json.dump(dig, f, indent=0, sort_keys=True)
        f.write('\n')
    print(path, len(dig), 'arrays')


if __name__ == '__main__':
    main()
