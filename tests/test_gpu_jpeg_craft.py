"""GPU: the device JPEG decoder (openpano_amd/csrc/jpeg_dec.hip) on streams that libjpeg's writer never produces (DESIGN.md
section 14.6).  The oracle is the serial restatement tests/harness/jpeg_dec_ref.c compiled here, which test_jpeg_craft_cpu.py
holds equal to libjpeg on every file; nothing here needs Pillow.

1. every file of tests/golden/jpeg_craft alone equals the restatement, at the default S, at 32 and at 64 bits;
2. the whole corpus in one batch, interleaved with five Pillow-written fixtures, at the default S and at 32 bits: table sets,
   samplings, interval counts and the number of k_jd_sync workgroups mixed in one call;
3. the two-bit file at S = 65536, where one subsequence completes about 32 000 blocks, with the round count read back;
4. the tile and run straddles at S = 32 as well (part of 1; named here because they are about k_jd_scan, not about S);
5. every corrupt file is OP_ERR_INVALID with its file index and the words of its error bit, alone and in the middle of a batch
   of good files; the pool holds what it held before, and a good file decodes afterwards;
6. files the parser refuses, in a batch: index and reason named, nothing allocated."""
import re

import numpy as np
import pytest

import jpeg_craft_cases as X
import jpeg_dec_cases as D
from openpano_amd import hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return D.build_ref(tmp_path_factory.mktemp("jpegcraftref"))


@pytest.fixture(scope="module")
def decoded(ref):
    """the restatement's pixels of every crafted file and of the Pillow fixtures mixed in, computed once and shared"""
    out = {n: D.ref_decode(ref, X.data(n)) for n in X.NAMES}
    for n in X.NAMES:
        assert D.digest(out[n]) == X.DIGESTS[n]["sha256"], n
    for n in X.PILLOW_MIX:
        out[n] = D.ref_decode(ref, D.data(n))
        assert D.digest(out[n]) == D.DIGESTS[n]["sha256"], n
    for a in out.values():
        a.setflags(write=False)
    return out


def _decode(ctx, files):
    v = hip.Views.decode_jpeg(ctx, files)
    try:
        assert v.count == len(files)
        return [v.numpy(i) for i in range(v.count)]
    finally:
        v.free()


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    diff = np.argwhere(got != want)
    assert len(diff) == 0, (what, len(diff), diff[:3].tolist())


@pytest.mark.parametrize("bits", [0, 32, 64], ids=["default", "S32", "S64"])
def test_every_file_alone(ctx, decoded, bits):
    ctx.set_jpeg_subseq_bits(bits)
    rounds = (0, None)
    try:
        for n in X.NAMES:
            _same(_decode(ctx, [X.data(n)])[0], decoded[n], (n, bits))
            rounds = max(rounds, (ctx.jpeg_last_rounds(), n))
    finally:
        ctx.set_jpeg_subseq_bits(0)
    print("largest round count at S =", bits or 1024, ":", rounds)


@pytest.mark.parametrize("bits", [0, 32], ids=["default", "S32"])
def test_whole_corpus_in_one_batch(ctx, decoded, bits):
    """at the default S k_jd_sync runs one workgroup per image; at 32 bits the batch's largest file has more than 2048
    subsequences and the intervals of every file are dealt over three workgroups, most of which find none to take"""
    names = list(X.NAMES)
    step = len(names) // len(X.PILLOW_MIX)
    for i, n in enumerate(X.PILLOW_MIX):
        names.insert(i * (step + 1) + step // 2, n)
    assert len(names) == len(X.NAMES) + 5
    files = [D.data(n) if n in X.PILLOW_MIX else X.data(n) for n in names]
    ctx.set_jpeg_subseq_bits(bits)
    try:
        for n, got in zip(names, _decode(ctx, files)):
            _same(got, decoded[n], ("batch", n, bits))
    finally:
        ctx.set_jpeg_subseq_bits(0)


def test_two_bit_blocks_at_the_largest_subsequence(ctx, decoded):
    ctx.set_jpeg_subseq_bits(65536)
    try:
        _same(_decode(ctx, [X.data(X.TWOBIT)])[0], decoded[X.TWOBIT], X.TWOBIT)
        rounds = ctx.jpeg_last_rounds()
        print("rounds of", X.TWOBIT, "at S = 65536:", rounds)
        assert rounds == 1           # two subsequences: the loop runs maxl - 1 = 1 round past pass A
    finally:
        ctx.set_jpeg_subseq_bits(0)


@pytest.mark.parametrize("bits", [0, 32], ids=["default", "S32"])
def test_straddles(ctx, decoded, bits):
    ctx.set_jpeg_subseq_bits(bits)
    try:
        names = X.STRADDLE_TILE + X.STRADDLE_RUN
        for n, got in zip(names, _decode(ctx, [X.data(n) for n in names])):
            _same(got, decoded[n], (n, bits))
    finally:
        ctx.set_jpeg_subseq_bits(0)


@pytest.mark.parametrize("what", sorted(X.CORRUPT))
def test_corrupt_files_are_answered(ctx, decoded, what):
    good, name = X.data("grey_hi_ids_rst1"), "grey_hi_ids_rst1"
    bad = X.corrupt(what)
    _decode(ctx, [good])
    before = hip.pool_stats()[:2]
    for bits in (0, 32):
        ctx.set_jpeg_subseq_bits(bits)
        try:
            for files in ([bad], [good, X.data("tables3_420"), bad, good, X.data("huff_skew_444")]):
                at = files.index(bad)
                with pytest.raises(hip.OpenPanoHipError, match=rf"error -1: op_views_decode_jpeg: file {at}: ") as e:
                    hip.Views.decode_jpeg(ctx, files)
                assert X.PHRASE[X.CORRUPT[what][0]] in str(e.value), (what, bits, str(e.value))
                assert hip.pool_stats()[:2] == before, (what, str(e.value))
            _same(_decode(ctx, [good])[0], decoded[name], "after " + what)
        finally:
            ctx.set_jpeg_subseq_bits(0)
    assert hip.pool_stats()[:2] == before


def test_parser_refusals_in_a_batch(ctx):
    good = X.data("shared_tables_444")
    _decode(ctx, [good])
    before = hip.pool_stats()
    for what, (code, why) in X.REFUSED.items():
        with pytest.raises(hip.OpenPanoHipError, match=rf"error {code}: op_views_decode_jpeg: file 2: .*{re.escape(why)}") as e:
            hip.Views.decode_jpeg(ctx, [good, X.data("tables3_422"), X.refused(what), good])
        assert hip.pool_stats() == before, (what, str(e.value))      # nothing allocated, nothing returned to the cache either
