"""Host side of the dropout streams (no GPU): ``DropoutStream`` as host state, the model attribute, and the argument checks
of rsaf_dropout_masks_group, which all run before anything touches a device (the pointers below are never dereferenced)."""
import pytest


def test_stream_is_host_state_with_a_two_key_state_dict():
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM, DropoutStream
    st = DropoutStream(2 ** 64 - 1)
    assert st.state_dict() == {"seed": 2 ** 64 - 1, "step": 0}
    st.load_state_dict({"seed": 9, "step": 2 ** 32 + 7})
    assert (st.seed, st.step) == (9, 2 ** 32 + 7) and DropoutStream(9, step=4).state_dict() == {"seed": 9, "step": 4}
    for bad in ({"seed": -1, "step": 0}, {"seed": 2 ** 64, "step": 0}, {"seed": 0, "step": -1}):
        with pytest.raises(ValueError):
            st.load_state_dict(bad)
    assert (st.seed, st.step) == (9, 2 ** 32 + 7)                      # a refused state changes nothing
    m = CNNLSTM(input_dim=16, cnn_out_channels=32, lstm_hidden_dim=64)
    keys = sorted(m.state_dict())
    assert m.dropout_stream is None and m.forced_masks is None
    m.dropout_stream = st
    assert sorted(m.state_dict()) == keys and not any(b is st for b in m.buffers())


def test_draw_masks_group_has_no_cpu_fallback(rsaf_lib):
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM, DropoutStream, draw_masks_group
    m = CNNLSTM(input_dim=16, cnn_out_channels=32, lstm_hidden_dim=64)
    st = DropoutStream(1)
    with pytest.raises(_lib.RsafError, match="no CPU fallback"):
        draw_masks_group([m], [(2, 7)], [st], "cpu")
    assert st.step == 0


def test_entry_checks_name_item_and_slot(rsaf_lib):
    from robust_speech_analysis_framework_amd import _lib

    def call(items, K=None):
        arr = (_lib.DropoutItem * max(len(items), 1))()
        for it, slots in zip(arr, items):
            it.seed, it.step = 1, 1
            for slot, (ptr, n, p) in slots.items():
                it.mask[slot], it.n[slot], it.p[slot] = ptr, n, p
        return rsaf_lib.rsaf_dropout_masks_group(arr, len(items) if K is None else K, None), rsaf_lib.rsaf_last_error().decode()

    base = 1 << 20
    ok = {0: (base, 8, 0.3)}
    assert call([], 0)[0] == 1 and call([ok] * 17)[0] == 1
    for items, where, text in [
            ([ok, {3: (base + 68, 8, 0.3)}], "item 1: slot 3:", "16-byte aligned"),
            ([ok, {2: (base + 64, 0, 0.3)}], "item 1: slot 2:", "n >= 1"),
            ([{4: (base, 8, 0.0)}], "item 0: slot 4:", "p > 0"),
            ([{4: (base, 8, -0.5)}], "item 0: slot 4:", "p > 0"),
            ([ok, {1: (base + 64, 8, float("nan"))}], "item 1: slot 1:", "NaN"),
            ([ok, {1: (None, -1, 0.0)}], "item 1: slot 1:", "n must be in [0, 2^32]"),
            ([ok, {1: (base + 64, 2 ** 32 + 1, 0.5)}], "item 1: slot 1:", "n must be in [0, 2^32]"),
            ([ok, {0: (base + 128, 8, 0.3), 5: (base + 16, 8, 0.3)}], "item 1: slot 5:", "overlaps the mask of item 0, slot 0"),
            ([{0: (base, 9, 0.3), 1: (base + 32, 8, 0.3)}], "item 0: slot 1:", "overlaps the mask of item 0, slot 0")]:
        rc, msg = call(items)
        assert rc == 1 and where in msg and text in msg, (items, rc, msg)
    # nothing drawn: RSAF_OK without a launch (there is no device here to launch on)
    assert call([{}, {0: (None, 0, 0.0), 5: (None, 12, 0.4)}])[0] == 0
