"""bench.py --dump-outputs without a GPU: the arrays of a stand-in EKF handle are written float64, bounded in size, and the sampled
instances are the same from run to run."""
import numpy as np

import bench


class _FakeEKF:
    def __init__(self, batch, L_max):
        self.batch, self.L_max, self.n_max = batch, L_max, 3 + 2 * L_max

    def get_state(self, b):
        M = b % (self.L_max + 1)
        n = 3 + 2 * M
        return dict(x=np.full(n, float(b)), P=np.full((n, n), float(b)), M=M, ids=np.arange(M, dtype=np.int32), timestep=0)

    def poses(self):
        return np.arange(3 * self.batch, dtype=np.float64).reshape(-1, 3)

    def truth(self):
        return -self.poses()

    def landmark_counts(self):
        return np.arange(self.batch, dtype=np.int32) % (self.L_max + 1)

    def status(self):
        return np.zeros(self.batch, dtype=np.int32)

    def error_stats(self):
        return np.linspace(0.0, 1.0, self.batch)


def test_dump_is_float64_bounded_and_seeded(tmp_path):
    for batch, L in ((16, 5), (65536, 50), (400000, 400)):
        a = bench.ekf_outputs(_FakeEKF(batch, L), first=1000)
        b = bench.ekf_outputs(_FakeEKF(batch, L), first=1000)
        assert set(a) == set(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
        assert all(v.dtype == np.float64 for v in a.values())
        assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BYTES_MAX
        nv = min(batch, bench.DUMP_VECTOR_INSTANCES)
        assert a["pose"].shape == (nv, 3) and a["instances"].shape == (nv,) and a["instances"][0] >= 1000
        ns = a["state_instances"].size
        assert 1 <= ns <= bench.DUMP_STATE_INSTANCES and a["state_P"].shape == (ns, 3 + 2 * L, 3 + 2 * L)
        # a state shorter than n_max is padded with NaN; its entries are the instance's own
        b0 = int(a["state_instances"][-1]) - 1000
        n = 3 + 2 * (b0 % (L + 1))
        assert np.all(a["state_x"][-1, :n] == b0) and np.all(np.isnan(a["state_x"][-1, n:]))
    bench.write_outputs(str(tmp_path / "out"), a)
    for k, v in a.items():
        assert np.array_equal(np.load(tmp_path / "out" / (k + ".npy")), v, equal_nan=True)
