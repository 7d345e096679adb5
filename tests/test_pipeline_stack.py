"""CPU-only: what tests/pipeline_stack.py claims of its scene, its parameters and its table, checked on the NumPy restatements alone,
so that no case of tests/test_gpu_pipeline_stack.py passes on a stage that has nothing to do: a stage that does nothing on the chosen
scene hides every ordering mistake around it."""

import numpy as np

import chromatic_spec
import pipeline_stack as ps
import temporal_spec

F = np.float32


def test_the_frames_hold_clipped_sites():
    """More than 100 and fewer than half the frame, at every call (the third is darker), in the plain decode and in the mosaic the
    highlight stage is given behind the three stages in front of it; and the stage rebuilds sites, above 1.0 too."""
    threshold = F(0.98)
    for name in ps.NAMES:
        chain = ps.sequence_chain(name)
        for call in range(ps.CALLS):
            plain = ps.decoded(ps.codes(name, call))
            prepared, filtered, corrected, balanced = chain[call]
            for what, mosaic in (('decoded', plain), ('prepared', prepared), ('in front of highlights', corrected)):
                clipped = int((mosaic >= threshold).sum())
                print(name, call, what, 'clipped sites', clipped)
                assert 100 < clipped < mosaic.size // 2, (name, call, what, clipped)
            gains = np.asarray(ps.GAINS, F)[ps.highlights_spec.colour_map(ps.H, ps.W, ps.highlights_spec.PATTERNS[ps.PATTERN])]
            white_balanced = np.fmin(np.fmax(corrected * gains, F(0)), F(1))
            assert (ps.bits(balanced) != ps.bits(white_balanced)).sum() > 100 and balanced.max() > 1.0
            out, total, cnt, chroma = ps.balanced(corrected)
            assert cnt.min() >= 64 and np.all(chroma != 0), (name, call, cnt)     # every colour has its offset: min_count is reached


def test_the_sensor_correction_acts():
    """Black levels, shading and both defect rules change the frame, and the defect rules fire on the planted sites."""
    black, scale = ps.rawprepare_spec.scale_of(ps.BLACK, ps.WHITE)
    for name in ps.NAMES:
        frame = ps.codes(name, 0)
        out, mask = ps.rawprepare_spec.raw_prepare_ref(frame, ps.PATTERN_WORD, black, scale, hot=True, dead=True, shading=ps.shading_grid(), clip=True)
        hot, dead = ps.DEFECTS[name]
        assert all(mask[s] == 1 for s in hot) and all(mask[s] == 2 for s in dead), (name, mask[tuple(zip(*hot))], mask[tuple(zip(*dead))])
        assert np.array_equal(ps.bits(out), ps.bits(ps.prepared(frame)))
        assert (ps.bits(out) != ps.bits(ps.decoded(frame))).mean() > 0.9
        assert out.min() >= 0 and out.max() == 1


def test_the_chromatic_model_moves_red_and_blue_at_a_corner():
    x0, y0, rn = ps.geometry()
    shifts = [chromatic_spec.corner_shift(row, x0, y0, rn, ps.W, ps.H) for row in ps.CA_MODEL]
    print('corner shifts in sites', shifts)
    assert all(abs(s) >= 0.5 for s in shifts) and shifts[0] * shifts[1] < 0      # red outwards, blue inwards
    assert all(abs(s) < chromatic_spec.MAX_SHIFT for s in shifts)                # the clamp does not act
    for name in ps.NAMES:
        prepared, filtered, corrected, _ = ps.sequence_chain(name)[1]
        moved = ps.bits(corrected) != ps.bits(filtered)
        colour = ps.highlights_spec.colour_map(ps.H, ps.W, ps.highlights_spec.PATTERNS[ps.PATTERN])
        assert not moved[colour == 1].any() and moved[colour == 0].mean() > 0.5 and moved[colour == 2].mean() > 0.5


def test_the_temporal_stage_has_a_history_after_the_second_frame():
    for name in ps.NAMES:
        state = temporal_spec.State((ps.H, ps.W))
        chain = ps.sequence_chain(name, state)
        assert np.array_equal(ps.bits(chain[0][1]), ps.bits(chain[0][0]))          # the first frame passes through by design
        assert not np.array_equal(ps.bits(chain[1][1]), ps.bits(chain[1][0]))      # the second is averaged with it
        again = temporal_spec.State((ps.H, ps.W))
        for call in range(2):
            temporal_spec.step(ps.prepared(ps.codes(name, call)), again, ps.NOISE_MODEL, temporal_spec.RGGB, max_frames=ps.MAX_FRAMES)
        share = float((again.next_read()[1] > 1).mean())
        print(name, 'share of sites with a count above 1 after the second frame', share)
        assert share > 0.5
        assert state.idx == ps.CALLS


def test_the_chains_run_and_are_deterministic():
    for name in ps.NAMES:
        a, b = ps.sequence_chain(name), ps.sequence_chain(name)
        assert len(a) == ps.CALLS
        for x, y in zip(a, b):
            for u, v in zip(x, y):
                assert u.dtype == F and u.shape == (ps.H, ps.W) and np.array_equal(ps.bits(u), ps.bits(v))
        assert not np.isnan(a[-1][3]).any()
    assert not np.array_equal(ps.sequence_chain('left')[0][3], ps.sequence_chain('right')[0][3])
    for call in range(ps.BRACKET_CALLS):
        (frames, merged, corrected, balanced), again = ps.bracket_chain(call), ps.bracket_chain(call)
        assert np.array_equal(ps.bits(balanced), ps.bits(again[3])) and balanced.dtype == F and balanced.shape == (ps.H, ps.W)
        clipped = [(f >= F(0.95)).mean() for f in frames]
        print('bracket', call, 'clipped share per exposure', clipped)
        assert clipped[0] > 0.1 and clipped[0] > 4 * clipped[2] > 0                 # the longest frame clips a tenth and more, the shortest its lights
        assert not np.array_equal(ps.bits(merged), ps.bits(frames[0]))              # the merge did something
        assert 100 < (corrected >= F(0.98)).sum() < corrected.size // 2             # and leaves clipped sites to the highlight stage
    assert not np.array_equal(ps.bracket_chain(0)[3], ps.bracket_chain(1)[3])


def test_the_payloads_unpack_to_the_codes():
    frame = ps.codes('left', 0)
    data = ps.payload(frame, ps.PADDING)
    assert data.dtype == np.uint8 and data.size == ps.W * ps.H * 3 // 2 + ps.PADDING and data[-ps.PADDING:].all()
    assert np.array_equal(ps.rawprepare_spec.unpack12(data[:-ps.PADDING], False, ps.H, ps.W), frame)
    assert frame.max() == 4095 and frame.min() < 100


def test_the_table_covers_every_raw_combination_and_every_stage(td):
    from torch_darktable.pipeline import ImageProcessor
    assert len(ps.RAW_CASES) == 64 == len(set(ps.RAW_CASES))
    for demosaic in ps.DEMOSAICS:
        for storage in ps.STORAGES:
            cases = ps.raw_cases(demosaic, storage)
            assert len({(c.temporal, c.raw_correction, c.chromatic, c.highlights) for c in cases}) == 16 == len(cases)
            assert len({ps.case_id(c) for c in cases}) == 16
    assert all((c.padding > 0) == c.raw_correction for c in ps.RAW_CASES)
    by = {c.white_balance_by for c in ps.RAW_CASES}
    assert by == {'highlights', 'apply_white_balance', 'raw_correction', 'fused'}
    assert [ps.case_id(c) for c in ps.RAW_CASES if c.white_balance_by == 'raw_correction'] == ['raw_correction'] * 4
    assert [ps.case_id(c) for c in ps.RAW_CASES if c.white_balance_by == 'fused'] == ['none'] * 2
    # a stage added to ImageProcessor later fails here until a configuration switches it on
    arguments, properties = ps.stage_names_of(ImageProcessor)
    print('constructor stages', arguments, 'property stages', properties)
    assert sorted(arguments) == sorted(ps.CONSTRUCTOR) and sorted(properties) == sorted(ps.PROPERTIES)
    missing = (set(arguments) | set(properties)) - ps.covered()
    assert not missing, missing
    assert set(ps.FRAME_STAGES) <= set(ps.FULL_STACK) and 'resize_width' in ps.FULL_STACK and 'hdr' in ps.BRACKET_STACK and 'temporal' not in ps.BRACKET_STACK
    assert set(ps.PLUMBING) - {'self'} <= set(__import__('inspect').signature(ImageProcessor.__init__).parameters)
