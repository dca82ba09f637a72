"""bench.py --dump-outputs (CPU): the pieces it samples are a function of the sizes alone, stay
inside the buffers and under the size limit, and the PCM unpacking is exact for each width."""
import numpy as np

import bench


def test_pieces_are_fixed_and_in_range():
    for n, head, run in ((8 << 30, bench.DUMP_HEAD, bench.DUMP_RUN), (1 << 20, bench.DUMP_FHEAD, bench.DUMP_FRUN),
                         (bench.DUMP_HEAD + 1, bench.DUMP_HEAD, bench.DUMP_RUN)):
        p = bench.dump_pieces(n, head, run, 7)
        assert p == bench.dump_pieces(n, head, run, 7)
        assert p[0] == (0, head) and len(p) == 1 + bench.DUMP_RUNS
        assert all(0 <= a < b <= n and b - a == min(run, n) for a, b in p[1:])
        assert p[1:] == sorted(p[1:])


def test_small_buffer_is_dumped_whole():
    assert bench.dump_pieces(100, bench.DUMP_HEAD, bench.DUMP_RUN, 7) == [(0, 100)]
    assert bench.dump_pieces(0, bench.DUMP_HEAD, bench.DUMP_RUN, 7) == [(0, 0)]


def test_dump_size_limit():
    pcm = (bench.DUMP_HEAD + bench.DUMP_RUNS * bench.DUMP_RUN) * 4        # float32: the 16- and 24-bit layouts
    info = (bench.DUMP_FHEAD + bench.DUMP_RUNS * bench.DUMP_FRUN) * len(bench.DUMP_INFO_FIELDS) * 8
    assert pcm + info <= 64 << 20


def test_unpack_pcm_exact():
    v16 = np.array([0, 1, -1, 32767, -32768], dtype="<i2")
    assert bench.unpack_pcm(v16.view(np.uint8), 2).tolist() == v16.tolist()
    v24 = np.array([0, 1, -1, 8388607, -8388608, 0x123456, -0x123456], dtype="<i4")
    raw = v24.view(np.uint8).reshape(-1, 4)[:, :3].reshape(-1).copy()
    out = bench.unpack_pcm(raw, 3)
    assert out.dtype == np.float32 and out.tolist() == v24.tolist()
    v32 = np.array([0, -1, 2**31 - 1, -2**31], dtype="<i4")
    out = bench.unpack_pcm(v32.view(np.uint8), 4)
    assert out.dtype == np.float64 and out.tolist() == v32.tolist()
