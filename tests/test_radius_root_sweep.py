"""The Box-Muller radius' square root with one residual correction (pocs_sqrt_radius) against the correctly rounded
expansion with two (pocs_sqrt_normal), on the DEVICE, for every argument the sampler can form.

The radius' argument t = |pocs_radius2_unit32(w)| takes 2^32 values, one per word, so the claim "the shorter root gives
sqrt()'s bits" is not argued from an error bound: pocs_probe_device_radius_roots forms t through the staged tables as the
sampling kernel does, takes both roots and counts the words whose bits differ.  All 2^32 words, 16 launches of 2^28."""
import pytest

CALLS = 16
PER_CALL = 1 << 28


@pytest.mark.gpu
def test_short_radius_root_equals_the_correctly_rounded_root_on_every_word(pocs):
    swept = 0
    with pocs.Context(0) as ctx:
        for i in range(CALLS):
            first = i * PER_CALL
            bad, first_bad = ctx.probe_device_radius_roots(first, PER_CALL)
            assert bad == 0, ("call %d: %d of the words [%d, %d) differ, the smallest 0x%08x" % (i, bad, first, first + PER_CALL, first_bad))
            swept += PER_CALL
    assert swept == 1 << 32


@pytest.mark.gpu
def test_radius_root_probe_refuses_a_range_past_the_last_word(pocs):
    with pocs.Context(0) as ctx:
        for first, count in ((0, 0), (1, 1 << 32), ((1 << 32) - 1, 2)):
            with pytest.raises(pocs.PocsError) as e:
                ctx.probe_device_radius_roots(first, count)
            assert e.value.code == -1
        assert ctx.probe_device_radius_roots((1 << 32) - 1, 1)[0] == 0        # the last word alone; the context still answers
        assert ctx.probe_device_radius_roots(0, 1)[0] == 0                    # the level 0 (a zero word)
