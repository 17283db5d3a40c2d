"""What the replay entries (csrc/replay.hip; tonic_buffer_* in csrc/offpolicy.hip) answer BEFORE any HIP call: every
invalid size, row or null pointer is TONIC_ERR_INVALID_ARGUMENT, and tonic_buffer_accumulate_n_steps with nothing to
fold is TONIC_OK without a launch.  One table; no GPU.

Every pointer is a fake non-NULL address that the host side never dereferences, and every call is shaped to return
before a launch (a launch would answer TONIC_ERR_LAUNCH on a machine without a GPU, never the status asserted here).
The method of tests/test_offpolicy_entries_host.py.
"""
import pytest

FAKE = 0x1000                     # a device pointer nobody reads
OK, INVALID = 0, -1

_SEG = ('d_seg_observations d_seg_actions d_seg_next_observations d_seg_rewards d_seg_resets d_seg_terminations '
        'd_seg_log_probs d_observations d_actions d_next_observations d_rewards d_resets d_terminations d_log_probs '
        'd_norm_acc row W O A stream')
_BUF = ('d_buf_observations d_buf_actions d_buf_next_observations d_buf_rewards d_buf_resets d_buf_terminations '
        'd_buf_discounts d_observations d_actions d_next_observations d_rewards d_resets d_terminations d_norm_acc '
        'row W O A discount_factor stream')
# entry -> its arguments in the order of include/tonic_hip.h: `d_*` a pointer, anything else a number from DEFAULTS
ENTRIES = {
    'tonic_meanstd_record': 'd_values d_norm_acc rows size stream',
    'tonic_segment_store': _SEG,
    'tonic_buffer_store': _BUF,
    'tonic_segment_gather': ('d_indices d_seg_observations d_seg_actions d_seg_advantages d_seg_log_probs '
                             'd_seg_returns d_observations d_actions d_advantages d_log_probs d_returns count '
                             'segment_rows O A stream'),
    'tonic_buffer_gather': ('d_indices d_buf_observations d_buf_actions d_buf_next_observations d_buf_rewards '
                            'd_buf_discounts d_observations d_actions d_next_observations d_rewards d_discounts W B '
                            'O A stream'),
    'tonic_buffer_accumulate_n_steps': ('d_buf_next_observations d_buf_rewards d_buf_discounts d_buf_resets '
                                        'd_next_observations d_rewards d_terminations row size max_size W O '
                                        'return_steps discount_factor stream'),
}
ENTRIES = {name: spec.split() for name, spec in ENTRIES.items()}
DEFAULTS = dict(rows=7, size=5, row=1, W=4, O=17, A=6, B=9, count=9, segment_rows=40, max_size=8, return_steps=3,
                discount_factor=0.99, stream=None)
# NULL is a valid d_norm_acc of the two stores: they then record nothing
OPTIONAL = {'tonic_segment_store': ('d_norm_acc',), 'tonic_buffer_store': ('d_norm_acc',)}


def call(lib, entry, **changes):
    """Calls `entry` with valid arguments but for `changes`; returns (status, tonic_last_error())."""
    values = dict(DEFAULTS, **changes)
    args = [values.get(name, FAKE) if name.startswith('d_') else values[name] for name in ENTRIES[entry]]
    return getattr(lib, entry)(*args), lib.tonic_last_error()


def invalid(lib, entry, **changes):
    status, error = call(lib, entry, **changes)
    assert status == INVALID, (entry, changes, status, error)
    assert entry.encode() in error, (entry, changes, error)


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    return _lib.load()


def test_every_entry_is_in_the_table():
    from tonic_amd import _lib
    for entry, names in ENTRIES.items():
        assert len(names) == len(_lib.SIGNATURES[entry][1]), entry


@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_each_null_pointer_is_an_invalid_argument(lib, entry):
    pointers = [name for name in ENTRIES[entry] if name.startswith('d_') and name not in OPTIONAL.get(entry, ())]
    assert len(pointers) >= 2
    for name in pointers:
        invalid(lib, entry, **{name: None})


def test_meanstd_record_sizes(lib):
    for changes in (dict(rows=0), dict(rows=-1), dict(size=0), dict(size=65), dict(size=-3)):
        invalid(lib, 'tonic_meanstd_record', **changes)


@pytest.mark.parametrize('entry', ['tonic_segment_store', 'tonic_buffer_store'])
def test_store_shapes_and_row(lib, entry):
    for changes in (dict(O=0), dict(O=1025), dict(O=-1), dict(W=0), dict(W=-2), dict(A=0), dict(A=-1), dict(row=-1)):
        invalid(lib, entry, **changes)
        invalid(lib, entry, d_norm_acc=None, **changes)       # (the form without a normaliser checks the same)


def test_segment_gather_counts(lib):
    for changes in (dict(count=0), dict(count=-1), dict(segment_rows=0), dict(segment_rows=-4), dict(O=0), dict(A=0)):
        invalid(lib, 'tonic_segment_gather', **changes)


def test_buffer_gather_counts_and_widths(lib):
    for changes in (dict(W=0), dict(W=-1), dict(B=0), dict(B=-1), dict(O=0), dict(O=-1), dict(A=0), dict(A=-1)):
        invalid(lib, 'tonic_buffer_gather', **changes)


def test_accumulate_n_steps_rows_and_sizes(lib):
    entry = 'tonic_buffer_accumulate_n_steps'
    for changes in (dict(row=8), dict(row=9), dict(row=-1), dict(size=9), dict(size=-1), dict(return_steps=0),
                    dict(return_steps=-2), dict(W=0), dict(O=0)):
        invalid(lib, entry, **changes)
    status, error = call(lib, entry, row=7, size=8, return_steps=0)       # the last valid row, a full buffer
    assert status == INVALID, error


def test_accumulate_n_steps_with_nothing_to_fold_is_ok_without_a_launch(lib):
    """back = min(size, return_steps - 1) == 0 (buffers.py:64: an empty loop): TONIC_OK, and no kernel — a launch
    answers TONIC_ERR_LAUNCH without a GPU, and with one these fake pointers must never reach a kernel."""
    entry = 'tonic_buffer_accumulate_n_steps'
    for changes in (dict(return_steps=1), dict(return_steps=1, size=8, row=7), dict(size=0), dict(size=0, row=0),
                    dict(size=0, return_steps=9)):
        status, error = call(lib, entry, **changes)
        assert status == OK, (changes, status, error)
