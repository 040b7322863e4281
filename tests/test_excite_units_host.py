"""CPU check of the work units of the persistent noise excitation (llsm_gpu_plan_index case 15): an utterance of ny
samples is cut into runs of one fixed length S from its first sample on, the last run shorter, and nothing else
enters -- so an utterance's units are the same alone and in any batch."""
import libllsm2_amd as llsm


def _units(L, ny):
    out = []
    while True:
        s0 = L.llsm_gpu_plan_index(15, ny, len(out), 0, 0.005, 44100.0, 4)
        if s0 < 0:
            return out
        out.append(s0)


def test_units_tile_each_utterance_in_runs_of_one_length():
    L = llsm.load()
    S = L.llsm_gpu_plan_index(15, 1 << 30, 1, 0, 0.005, 44100.0, 4)
    assert 512 <= S <= 2048
    assert _units(L, 0) == []
    for ny in (1, S - 1, S, S + 1, 7001, 19999, 20000, 20131, 44100, 68355, 150000):
        s = _units(L, ny)
        assert s == [k * S for k in range((ny + S - 1) // S)], ny
        assert L.llsm_gpu_plan_index(15, ny, -1, 0, 0.005, 44100.0, 4) == -1
