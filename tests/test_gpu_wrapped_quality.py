"""The quality strings of wrapped FASTQ records on the device (crass_hip_fetch_quality_device(_to) with FASTQ class 1 on the
context: k_qw_measure) against the reader's qual (crass_read_fastx), for wrapped and four-line files: all records, a shuffled
subset with duplicates, into a caller's device buffer whose neighbours stay untouched.  Every comparison is exact equality."""
import numpy as np
import pytest

from tests import wrapped_sets

pytestmark = pytest.mark.gpu

T = 4096
DESIGNED = wrapped_sets.designed(T)
NAMES = ["wrap1", "wrap7", "wrap60", "line_of_4097", "quality_starts_with_at_and_plus", "crlf", "void_lines", "void_lines_inside", "blanks_in_lines",
         "empty_then_void", "empty_at_end", "no_final_newline", "read_9000_wrap60", "qual_last_byte_of_tile", "records_1025",
         "quality_lines_look_like_headers", "four_line", "four_line_empty_reads"]


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


@pytest.fixture(scope="module")
def eng(ca):
    with ca.SearchEngine() as e:
        e.set_fastq_class(1)
        yield e


def reader_quality(ca, tmp_path, data):
    p = tmp_path / "in.fq"
    p.write_bytes(data)
    f = ca.FastxFile(str(p))
    qual, off = f.qual.tobytes(), f.qual_off.astype(np.int64)
    return [qual[off[r]:off[r + 1]] for r in range(f.n_reads)]


@pytest.mark.parametrize("name", NAMES)
def test_quality_equals_the_readers(ca, eng, tmp_path, name):
    import torch
    data = DESIGNED[name]
    want = reader_quality(ca, tmp_path, data)
    assert want == [q for _, _, q in wrapped_sets.records(data)], name
    lay = eng.load_fastx_bytes(data, pad_uniform=2)
    assert lay.n_reads == len(want)
    dev = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    rng = np.random.RandomState(5)
    n = lay.n_reads
    picks = [np.arange(n), rng.randint(0, n, size=min(2 * n, 300) + 3)]
    for idx in picks:
        chars, off, has = eng.fetch_quality(dev, len(data), lay.rec_pos, idx)
        assert has.tolist() == [1] * len(idx)
        got = [chars[int(off[k]):int(off[k + 1])].tobytes() for k in range(len(idx))]
        assert got == [want[int(r)] for r in idx], name
        total = int(off[-1])
        out = torch.full((total + 32,), 0xEE, dtype=torch.uint8, device="cuda")
        _, off2, has2 = eng.fetch_quality(dev, len(data), lay.rec_pos, idx, out=out[16:16 + total])
        back = out.cpu().numpy()
        assert np.array_equal(off2, off) and np.array_equal(has2, has)
        assert back[16:16 + total].tobytes() == b"".join(got) and np.all(back[:16] == 0xEE) and np.all(back[16 + total:] == 0xEE), name


def test_four_line_records_get_the_same_answer_under_both_classes(ca, eng, tmp_path):
    import torch
    data = DESIGNED["four_line"]
    lay = eng.load_fastx_bytes(data, pad_uniform=2)
    dev = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    idx = np.arange(lay.n_reads)[::-1].copy()
    a = eng.fetch_quality(dev, len(data), lay.rec_pos, idx)
    with ca.SearchEngine() as e4:
        e4.load_fastx_bytes(data, pad_uniform=2)
        b = e4.fetch_quality(dev, len(data), lay.rec_pos, idx)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
