"""GPU decodes of the damaged streams of tests/golden/manifest_damage.json
(oracle/make_golden_damage.py: 1 to 3 bytes of a golden replaced inside its
tile-parts, decoded by the reference) against the reference's results: an
error exactly where it refuses, otherwise the same image (SHA-256 of the
decoded planes, tolerance 0) -- from Codec.decompress, from
Codec.decompress_batch in lists of 32 with the refusals mixed in, and from the
batch Tier-1 kernels without the work sort.

Nothing here is meant to reach a device with a bad table: before a stream is
decoded, the tables the host half would hand the kernels
(grkgpu_dec_tables_of) are checked on the host (damage_fixtures.plan_problems)
and a stream that fails the check is reported without being decoded."""
import functools

import pytest

import damage_fixtures as dmg

pytestmark = pytest.mark.gpu


def _grk():
    import grokimagecompression_amd as grk
    return grk


@functools.lru_cache(maxsize=None)
def guarded(name):
    """[(case, damaged stream, host accepts)] of stream `name`; a stream whose
    tables do not pass the host checks fails the test here, undecoded"""
    grk = _grk()
    out, unsafe = [], []
    for c, cs in dmg.cases(name):
        try:
            bad = dmg.plan_problems(grk.dec_tables(cs))
        except grk.GrkGpuError:
            out.append((c, cs, False))
            continue
        if bad:
            unsafe.append((c["p"], bad))
        out.append((c, cs, True))
    assert not unsafe, (name, len(unsafe), unsafe[:4])
    return out


def decode_single(codec, name, cases=None):
    """sha256 of each case's decode, None where the decode fails"""
    grk = _grk()
    got = []
    for c, cs, ok in (cases or guarded(name)):
        if not ok:  # refused on the host: the same call, no device work
            with pytest.raises(grk.GrkGpuError):
                codec.decompress(cs)
            got.append(None)
            continue
        try:
            got.append(dmg.planes_sha(codec.decompress(cs)))
        except grk.GrkGpuError:
            got.append(None)
    return got


def clean_still_decodes(codec, name):
    """the codec is healthy: the clean stream decodes to the reference's image"""
    assert dmg.planes_sha(codec.decompress(dmg.clean(name))) == dmg.manifest()[name]["clean"], name


@pytest.mark.parametrize("name", dmg.STREAMS)
def test_damaged_stream_matches_reference(codec, name):
    """Codec.decompress and Codec.decompress_batch[_convert] of every case."""
    grk = _grk()
    cases = guarded(name)
    single = decode_single(codec, name)
    wrong = []
    for (c, cs, ok), sha in zip(cases, single):
        want = None if c["r"] == "error" else c["r"]
        if sha != want:
            wrong.append((c["p"], c["s"], "refused" if sha is None else "decoded",
                          "the reference refuses" if want is None else "the reference decodes"
                          if sha is None else "another image"))
    assert not wrong, (name, len(wrong), wrong[:8])
    clean_still_decodes(codec, name)
    # the same streams in lists of 32, refusals mixed in: each item its single call's result
    batch = codec.decompress_batch_convert if name.startswith("sub_") else codec.decompress_batch
    for i0 in range(0, len(cases), 32):
        part = cases[i0:i0 + 32]
        outs = batch([cs for c, cs, ok in part], errors="return")
        assert len(outs) == len(part)
        for j, o in enumerate(outs):
            sha = None if isinstance(o, grk.GrkGpuError) else dmg.planes_sha(o)
            assert sha == single[i0 + j], (name, part[j][0]["p"], "batch item differs from the single call")
        assert codec.batch_info["n_ok"] == sum(s is not None for s in single[i0:i0 + 32])
    clean_still_decodes(codec, name)


@pytest.mark.parametrize("name", ["rgb12_M46_tiles", "g8_sop_eph"])
@pytest.mark.parametrize("opts", [dict(t1_dec_sort=0), dict(t1_lone=-1)], ids=["unsorted", "batch_t1"])
def test_plan_variants(codec, name, opts):
    """One stream with tiles and one without, the block table left in stream
    order and through the batch Tier-1 kernels: the same images."""
    grk = _grk()
    cases = guarded(name)
    with grk.dwt_options(**opts):
        got = decode_single(codec, name)
    want = [None if c["r"] == "error" else c["r"] for c, cs, ok in cases]
    diff = [(c["p"], c["s"]) for (c, cs, ok), g, w in zip(cases, got, want) if g != w]
    assert not diff, (name, opts, len(diff), diff[:8])
    clean_still_decodes(codec, name)
