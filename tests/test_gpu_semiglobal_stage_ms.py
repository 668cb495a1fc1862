"""gw_aligner_stage_ms (CudaAlignerBatch.stage_ms), the HIP-event times that tools/bench_semiglobal.py reports: nothing
before align_all(), two non-negative times after it, nothing for a global aligner."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

CACHE = 1 << 30


@pytest.mark.parametrize("mode", ["infix", "prefix"])
def test_stage_times_follow_align_all(mode):
    from genomeworks_amd import cudaaligner
    al = cudaaligner.CudaAlignerBatch(100, 300, 4, alignment_type=mode, max_device_memory_allocator_caching_size=CACHE)
    with pytest.raises(RuntimeError, match="no align_all"):
        al.stage_ms()
    ends, traceback = C.c_float(-2), C.c_float(-2)
    assert al._L.gw_aligner_stage_ms(al._h, C.byref(ends), C.byref(traceback)) == -1
    assert (ends.value, traceback.value) == (-2, -2)            # an error leaves the outputs alone
    # one pair with a slice to trace back, one without (its traceback stage is empty)
    for q, t in (("ACGTACGTAC", "TTTTACGTACGGACTTTT"), ("AAAA", "CCCC")):
        assert al.add_alignment(q, t) == 0
    al.align_all()
    assert al.sync() == 2
    ends_ms, traceback_ms = al.stage_ms()
    assert 0 <= ends_ms < 1000 and 0 <= traceback_ms < 1000
    assert al._L.gw_aligner_stage_ms(al._h, None, None) == 0     # either output may be left out


def test_global_aligners_have_no_stages():
    from genomeworks_amd import cudaaligner
    for kw in ({}, {"max_bandwidth": 64}):
        al = cudaaligner.CudaAlignerBatch(100, 100, 2, max_device_memory_allocator_caching_size=CACHE, **kw)
        assert al.add_alignment("ACGT", "ACGGT") == 0
        al.align_all()
        assert al.sync() == 1
        with pytest.raises(RuntimeError, match="not an infix / prefix aligner"):
            al.stage_ms()
