"""Part of bench.py (repo root): --dump-outputs, what the timed path returned in its last step, written for a comparison
between two builds.  bench.py re-exports these names."""
import os

DUMP_CAP_BYTES = 64 * 10 ** 6


def dump_outputs(dirname, tensors, cap_bytes=DUMP_CAP_BYTES):
    """{name: tensor} -> dirname/<name>.npy, float32, at most cap_bytes in all.  An output over its share of the cap is
    written as a sample of its flattened elements at sorted positions drawn with a fixed seed: the same positions in every
    run of the same shape, so that two dumps still compare element for element."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    share = cap_bytes // 4 // max(len(tensors), 1)
    for name, t in tensors.items():
        x = t.detach().float().cpu().numpy()
        if x.size > share:
            pos = np.sort(np.random.default_rng(0).choice(x.size, size=share, replace=False))
            x = x.reshape(-1)[pos]
        np.save(os.path.join(dirname, name + ".npy"), np.ascontiguousarray(x, dtype=np.float32))
