"""epoch.epoch_batches - the (first pick, size) list of a staged sequence of epochs (FusedPCGNN.stage_epoch walks it) - against a
plain double loop.  No GPU."""
import pytest

from pcgnn_amd.epoch import epoch_batches

SHAPES = [(1, 1, 1), (5, 8, 1),      # one short batch
          (512, 256, 1),             # an exact multiple
          (513, 256, 1),
          (700, 256, 3),             # a short last batch in every epoch
          (256, 256, 2)]


def double_loop(n, batch_size, n_epochs):
    out = []
    for e in range(n_epochs):
        b = 0
        while b * batch_size < n:
            out.append((e * n + b * batch_size, min(batch_size, n - b * batch_size)))
            b += 1
    return out


@pytest.mark.parametrize("n,batch_size,n_epochs", SHAPES)
def test_epoch_batches(n, batch_size, n_epochs):
    got = epoch_batches(n, batch_size, n_epochs)
    assert got == double_loop(n, batch_size, n_epochs)
    per_epoch = -(-n // batch_size)
    assert len(got) == n_epochs * per_epoch
    for e in range(n_epochs):
        epoch = got[e * per_epoch:(e + 1) * per_epoch]
        assert sum(size for _, size in epoch) == n
        assert [first for first, _ in epoch] == [e * n + b * batch_size for b in range(per_epoch)]
        assert all(size == batch_size for _, size in epoch[:-1]) and 0 < epoch[-1][1] <= batch_size
