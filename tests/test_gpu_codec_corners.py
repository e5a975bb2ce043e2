"""The four device codecs (DESIGN.md sections 10, 12, 13, 14) on the GPU at their crafted corners: the bodies of
tests/test_codec_corners.py with the device as the codec and the device's own read pass as the source of its results
(amp_sam_process, deferred with BAM output, and amp_bam_process).  The expectation is the Python codec's with the oracle's
results; no twin is built.  One Engine, one SamCodec and one BamCodec serve the module; every step runs once."""
import pytest

from amplipy_amd import bam_device, lib, sam_native
from tests import codec_corners as K
from tests import sam_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    mn, mx, mpl = lib.find_overlapping_primers(K.G.size, [(s, e) for s, e, _ in K.PRIMERS], 0)
    eng = lib.Engine(K.G.size)
    eng.set_primers(mn, mx, mpl)
    eng.set_params(K.MIN_QUALITY, K.WINDOW, True, False)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def sam(engine):
    c = sam_native.SamCodec(engine)
    c.set_references(U.ref_names(K.HDR))
    yield c
    c.close()


@pytest.fixture(scope="module")
def bam(engine):
    c = bam_device.BamCodec(engine)
    c.set_references([n for n, _ in K.BAM_HDR.refs])
    yield c
    c.close()


def give(codec, res, verdict, read_base):
    return codec.process(read_base)


def give_deferred(codec, res, verdict, read_base):
    return codec.process(read_base, defer=True)           # the verdict comes down with the encode


def test_sam_text_good_lines(sam):
    """Batch = the Python packer's, pads included; text = the Python writer's with the oracle's results; counters equal;
    first_odd_line -1 (all in check_sam_text)."""
    K.sam_text_good(sam, give)


def test_sam_to_bam_good_lines(sam):
    """Stream = python_stream, the blocks inflate to it, no host block and one wait per encode (check_sam_bam)."""
    K.sam_bam_good(sam, give_deferred)


def test_bam_corners_to_text_and_to_bam(bam, tmp_path):
    K.bam_corners(bam, give, tmp_path)


def test_rows_with_a_status(engine, sam, bam, tmp_path):
    K.rows_with_a_status(sam, bam, give, give_deferred, give, tmp_path)
    engine.set_params(K.MIN_QUALITY, K.WINDOW, True, True)
    try:
        K.rows_with_a_counting_status(sam, give, give_deferred)
    finally:
        engine.set_params(K.MIN_QUALITY, K.WINDOW, True, False)


def test_odd_means_odd(sam, bam, tmp_path):
    K.odd_lines_text(sam)
    K.odd_lines_bam_out(sam)
    K.odd_records(bam, tmp_path)


def test_floats(sam, bam, tmp_path):
    """The device's fp64 multiply, divide and narrowing cast against CPython's float(); its 64-bit integer '%g' against CPython's."""
    K.floats(sam, bam, give_deferred, give, tmp_path)


def test_one_codec_many_shapes(sam):
    K.one_codec_many_shapes(sam, give, give_deferred)
