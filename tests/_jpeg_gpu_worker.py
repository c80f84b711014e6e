"""Child process of tests/test_gpu_jpeg.py: ``Engine.jpeg_decode`` over the packed tiles of ``argv[1]`` (npz: scan, desc, tables,
px), tiles and status words to ``argv[2]``.  The parent gives it a time limit: a kernel that did not come back ends with the
child, not with the test session."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main():
    import torch
    from biscuit_amd.engine import Engine
    from biscuit_amd.weights import synthetic_weights
    d = np.load(sys.argv[1])
    eng = Engine(synthetic_weights(1), dtype='f16', max_batch=8, max_mc=2)
    tiles, status = eng.jpeg_decode(torch.from_numpy(d['scan']).cuda(), torch.from_numpy(d['desc'].view(np.int32)).cuda(),
                                    torch.from_numpy(d['tables']).cuda(), int(d['px']))
    torch.cuda.synchronize()
    np.savez(sys.argv[2], tiles=tiles.cpu().numpy(), status=status.cpu().numpy())


if __name__ == '__main__':
    main()
