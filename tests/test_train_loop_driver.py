"""train._run_batches, the batch driver of train()'s ring-logged native loops, on the host: fake launch / fetch / bookkeep
callables log their calls and model the device ring (a launch writes iteration it into slot it mod R, a fetch checks that the
slots of its batch still hold that batch)."""
import pytest

from depth_correction_amd.train import _run_batches


class FakeLoop:
    """A loop over a ring of R slots.  Once ``left`` allows, a launch starts G iterations (a captured graph's replay).  ``refuse``:
    the iteration whose launch is refused; ``abandon``: the (first, upto) whose fetch returns None; ``fail``: the calls, as in the
    log, that raise KeyboardInterrupt the first time they are made."""

    def __init__(self, R, G=1, refuse=None, abandon=None, fail=()):
        self.R, self.G, self.refuse, self.abandon, self.fail = R, G, refuse, abandon, set(fail)
        self.ring = R * [None]
        self.log = []

    def _interrupt(self, name):
        if name in self.fail:
            self.fail.discard(name)
            raise KeyboardInterrupt

    def launch(self, it, left):
        self._interrupt('L%d' % it)
        if it == self.refuse:
            self.log.append('R%d' % it)
            return 0
        n = self.G if left >= self.G else 1
        for q in range(it, it + n):
            self.ring[q % self.R] = q
        self.log.append('L%d' % it if n == 1 else 'L%d+%d' % (it, n))
        return n

    def fetch(self, first, upto):
        self.log.append('F%d:%d' % (first, upto))
        self._interrupt('F%d:%d' % (first, upto))
        if (first, upto) == self.abandon:
            return None
        rows = [self.ring[i % self.R] for i in range(first, upto)]
        assert rows == list(range(first, upto)), 'a slot of the batch was overwritten'
        return rows

    def bookkeep(self, fetched, first, upto):
        assert fetched == list(range(first, upto))
        self.log.append('B%d:%d' % (first, upto))
        self._interrupt('B%d:%d' % (first, upto))

    def run(self, n_it, sharded=False):
        return _run_batches(n_it, self.R, self.launch, self.fetch, self.bookkeep, sharded)


def _launches(first, upto):
    return ['L%d' % i for i in range(first, upto)]


@pytest.mark.parametrize('n_it, R, want', [
    (3, 4, _launches(0, 3) + ['F0:3', 'B0:3']),
    (4, 4, _launches(0, 4) + ['F0:4', 'B0:4']),
    (6, 4, _launches(0, 4) + ['F0:4'] + _launches(4, 6) + ['B0:4', 'F4:6', 'B4:6']),
    (9, 4, _launches(0, 4) + ['F0:4'] + _launches(4, 8) + ['B0:4', 'F4:8', 'L8', 'B4:8', 'F8:9', 'B8:9']),
    (3, 1, ['L0', 'F0:1', 'L1', 'B0:1', 'F1:2', 'L2', 'B1:2', 'F2:3', 'B2:3']),
])
def test_batches_fetch_before_launching_and_bookkeep_while_the_next_runs(n_it, R, want):
    loop = FakeLoop(R)
    assert loop.run(n_it) is True
    assert loop.log == want
    assert sum(e.startswith('F') for e in loop.log) == -(-n_it // R)          # one synchronisation per batch


@pytest.mark.parametrize('n_it, R, G, want', [
    # G divides R: whole replays, single launches for a tail shorter than G
    (19, 8, 4, ['L0+4', 'L4+4', 'F0:8', 'L8+4', 'L12+4', 'B0:8', 'F8:16', 'L16', 'L17', 'L18', 'B8:16', 'F16:19', 'B16:19']),
    # G does not divide R: a replay never runs past the end of its batch
    (10, 8, 3, ['L0+3', 'L3+3', 'L6', 'L7', 'F0:8', 'L8', 'L9', 'B0:8', 'F8:10', 'B8:10']),
])
def test_launches_of_several_iterations_stay_inside_their_batch(n_it, R, G, want):
    loop = FakeLoop(R, G)
    assert loop.run(n_it) is True
    assert loop.log == want


def test_a_refused_first_launch_means_the_loop_did_not_run():
    loop = FakeLoop(4, refuse=0)
    assert loop.run(8) is False
    assert loop.log == ['R0']


def test_a_sharded_refusal_raises_even_at_the_first_iteration():
    loop = FakeLoop(4, refuse=0)
    with pytest.raises(RuntimeError, match='refused the native step'):
        loop.run(8, sharded=True)
    assert loop.log == ['R0']


def test_a_later_refusal_raises_and_keeps_the_fetched_batch():
    loop = FakeLoop(4, refuse=5)
    with pytest.raises(RuntimeError, match='refused the native step'):
        loop.run(8)
    assert loop.log == _launches(0, 4) + ['F0:4', 'L4', 'R5', 'B0:4']


def test_an_abandoned_fetch_ends_the_run_without_bookkeeping():
    loop = FakeLoop(4, abandon=(4, 8))
    assert loop.run(12) is True
    assert loop.log == _launches(0, 4) + ['F0:4'] + _launches(4, 8) + ['B0:4', 'F4:8']


@pytest.mark.parametrize('sharded', [False, True])
def test_an_interrupt_keeps_a_batch_already_fetched(sharded):
    """Interrupted after the batch 4..7 was fetched and part of the next one launched (its first slot is overwritten now): the
    records on the host are bookkept, and nothing is read from the ring again.  Sharded runs keep nothing."""
    loop = FakeLoop(4, fail={'L9'})
    with pytest.raises(KeyboardInterrupt):
        loop.run(12, sharded=sharded)
    head = _launches(0, 4) + ['F0:4'] + _launches(4, 8) + ['B0:4', 'F4:8', 'L8']
    assert loop.log == head + ([] if sharded else ['B4:8'])


@pytest.mark.parametrize('sharded', [False, True])
def test_an_interrupted_fetch_is_repeated_when_nothing_of_the_next_batch_was_launched(sharded):
    loop = FakeLoop(4, fail={'F4:8'})
    with pytest.raises(KeyboardInterrupt):
        loop.run(12, sharded=sharded)
    head = _launches(0, 4) + ['F0:4'] + _launches(4, 8) + ['B0:4', 'F4:8']
    assert loop.log == head + ([] if sharded else ['F4:8', 'B4:8'])


def test_an_interrupt_at_the_last_fetch_keeps_the_last_batch():
    loop = FakeLoop(4, fail={'F4:6'})
    with pytest.raises(KeyboardInterrupt):
        loop.run(6)
    assert loop.log == _launches(0, 4) + ['F0:4'] + _launches(4, 6) + ['B0:4', 'F4:6', 'F4:6', 'B4:6']


@pytest.mark.parametrize('sharded', [False, True])
def test_an_interrupt_inside_the_bookkeeping_bookkeeps_the_batch_again(sharded):
    """The batch's records are still on the host: they are bookkept from the start once more, so the batch's checkpoint is
    written (its progress lines are printed twice).  Sharded runs keep nothing."""
    loop = FakeLoop(4, fail={'B0:4'})
    with pytest.raises(KeyboardInterrupt):
        loop.run(12, sharded=sharded)
    head = _launches(0, 4) + ['F0:4'] + _launches(4, 8) + ['B0:4']
    assert loop.log == head + ([] if sharded else ['B0:4'])
