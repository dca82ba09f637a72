"""Host side of bnflac_index_streams: the descriptor table and its check (no GPU)."""
import ctypes

import numpy as np
import pytest

from birdnest.audio_amd import libflac


def test_stream_desc_layout():
    assert ctypes.sizeof(libflac.StreamDesc) == 32
    assert [f[0] for f in libflac.StreamDesc._fields_] == list(libflac.STREAM_DESC_DTYPE.names)
    assert libflac.STREAM_DESC_DTYPE.itemsize == 32
    assert "bnflac_index_streams" in libflac.BATCH_SYMBOLS


def test_stream_table_values():
    t = libflac.stream_table([(0, 10, 4, 100), (10, 10, 10, 0), (13, 40, 20, 7)], 40)
    assert t.view(np.uint64).reshape(-1, 4).tolist() == [[0, 10, 4, 100], [10, 10, 10, 0], [13, 40, 20, 7]]
    assert len(libflac.stream_table([], 0)) == 0


@pytest.mark.parametrize("streams", [
    [(5, 4, 5, 0)],                   # begin > end
    [(0, 41, 0, 0)],                  # end > nbytes
    [(2, 10, 1, 0)],                  # first_offset before begin
    [(2, 10, 11, 0)],                 # first_offset past end
    [(0, 10, 0, 0), (9, 20, 9, 0)],   # overlapping
    [(10, 20, 10, 0), (0, 5, 0, 0)],  # out of order
])
def test_stream_table_rejects(streams):
    with pytest.raises(ValueError):
        libflac.stream_table(streams, 40)
