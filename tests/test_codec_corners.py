"""The gate in front of tests/test_gpu_codec_corners.py: every check function of tests/codec_corners.py with a host twin as the
codec, the oracle's results handed to it through twin_set_results / set_trim.  Proves without a GPU that the corpora, their
good / failing partitions and the Python codec's expectations agree with each other and with the twins; the GPU module changes
the codec argument (and how the codec gets its results) only."""
import os
import shutil

import pytest

from amplipy_amd import bam_device
from tests import codec_corners as K
from tests import sam_util as U
from tests.test_bam_reencode_twin import deflater, twin as bam_twin_so        # noqa: F401 (fixtures)
from tests.test_sam_to_bam_twin import new_twin

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")),
                                reason="g++ and hipcc needed to build the twins")


@pytest.fixture(scope="module")
def sam(tmp_path_factory, deflater):        # noqa: F811
    c = new_twin(U.twin_path(tmp_path_factory.mktemp("twin")), deflater)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bam(bam_twin_so, deflater):        # noqa: F811
    c = bam_device.BamCodec(twin=bam_twin_so)
    c.set_deflater(deflater)
    c.set_references([n for n, _ in K.BAM_HDR.refs])
    yield c
    c.close()


def give_sam(codec, res, verdict, read_base):
    return codec.twin_set_results(res)


def give_bam(codec, res, verdict, read_base):
    codec.set_trim(res, first_bad=verdict[0])
    return verdict


def test_every_line_is_good_or_failing_and_the_primer_rows_change():
    t, b, r = K.text_corpus(), K.bam_corpus(), K.recs_corpus()               # (the partitions and primer_effects assert inside)
    assert len(t["hand"]) + len(K.FAILING["hand"]) == len(K.ST.hand_written_lines())
    assert len(t["length"]) + len(K.FAILING["length"]) == len(K.length_lines())
    assert len(b["corner"]) + len(K.FAILING["corner"]) == len(K.SB.corner_lines())
    assert len(r["corner"]) + len(K.RECS_FAILING) == len(K.BT.corner_recs())
    assert {st for _, st in t["failing"]} == {1, 6, 8} and {st for _, st in b["failing"]} == {1, 6} and {st for _, st in r["failing"]} == {1, 6, 8}
    for n in K.BASE_LENGTHS[1:]:                                            # the CRLF lines: CR on a slot's last byte, LF on the next one's first
        l = K.crlf_line(n, 100)
        assert l.endswith(b"\r\n") and (len(l) - 1) % 16 == 0


def test_sam_text_good_lines(sam):
    K.sam_text_good(sam, give_sam)


def test_sam_to_bam_good_lines(sam):
    K.sam_bam_good(sam, give_sam)


def test_bam_corners_to_text_and_to_bam(bam, tmp_path):
    K.bam_corners(bam, give_bam, tmp_path)


def test_rows_with_a_status(sam, bam, tmp_path):
    K.rows_with_a_status(sam, bam, give_sam, give_sam, give_bam, tmp_path)
    K.rows_with_a_counting_status(sam, give_sam, give_sam)


def test_odd_means_odd(sam, bam, tmp_path):
    K.odd_lines_text(sam)
    K.odd_lines_bam_out(sam)
    K.odd_records(bam, tmp_path)


def test_floats(sam, bam, tmp_path):
    K.floats(sam, bam, give_sam, give_bam, tmp_path)


def test_one_codec_many_shapes(sam):
    K.one_codec_many_shapes(sam, give_sam, give_sam)
