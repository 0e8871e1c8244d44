"""GPT2.forward(..., doc_ids=...) on the CPU: the document mask and the
per-document position reset together make packed documents exactly
independent of each other."""

import sys

import pytest
import torch
from torch.nn import functional as F

from dmlcloud_amd.models import gpt2_tiny

T = 48
# two rows, three documents each, as (start, end) pairs
ROWS = [[(0, 10), (10, 30), (30, 48)], [(0, 1), (1, 25), (25, 48)]]


def _batch():
    g = torch.Generator().manual_seed(0)
    idx = torch.randint(0, 512, (len(ROWS), T), generator=g)
    targets = torch.randint(0, 512, (len(ROWS), T), generator=g)
    doc_ids = torch.empty(len(ROWS), T, dtype=torch.int64)
    for r, docs in enumerate(ROWS):
        for d, (lo, hi) in enumerate(docs):
            doc_ids[r, lo:hi] = 100 + d  # any run of equal values is a document
    return idx, targets, doc_ids


def _model():
    torch.manual_seed(1)
    return gpt2_tiny()


def test_packed_logits_equal_each_document_alone():
    model = _model()
    idx, _, doc_ids = _batch()
    with torch.no_grad():
        packed = model(idx, doc_ids=doc_ids)
        for r, docs in enumerate(ROWS):
            for lo, hi in docs:
                alone = model(idx[r : r + 1, lo:hi])
                torch.testing.assert_close(packed[r : r + 1, lo:hi], alone, rtol=0.0, atol=1e-4)


def test_packed_gradients_equal_sum_over_documents():
    idx, targets, doc_ids = _batch()

    packed_model = _model()
    logits = packed_model(idx, doc_ids=doc_ids)
    F.cross_entropy(logits.view(-1, logits.size(-1)), targets.view(-1), reduction='sum').backward()

    alone_model = _model()
    for r, docs in enumerate(ROWS):
        for lo, hi in docs:
            logits = alone_model(idx[r : r + 1, lo:hi])
            loss = F.cross_entropy(logits.view(-1, logits.size(-1)), targets[r, lo:hi], reduction='sum')
            loss.backward()  # accumulates: the sum over the separate runs

    for (name, p), (_, p2) in zip(packed_model.named_parameters(), alone_model.named_parameters()):
        assert p.grad is not None, name
        # summed-loss gradients reach ~10 in magnitude; 1e-4 relative on top
        # of the 1e-4 absolute the logits get
        torch.testing.assert_close(p.grad, p2.grad, rtol=1e-4, atol=1e-4, msg=lambda m: f'{name}: {m}')


def test_without_doc_ids_nothing_changes():
    model = _model()
    idx, targets, _ = _batch()
    with torch.no_grad():
        a = model(idx)
        b = model(idx, doc_ids=None)
        assert torch.equal(a, b)
        la, loss_a = model(idx, targets)
        lb, loss_b = model(idx, targets, None)
        assert torch.equal(la, lb) and torch.equal(loss_a, loss_b)


def test_one_document_equals_no_doc_ids():
    """A single document per row is plain causal attention with plain
    positions."""
    model = _model()
    idx, _, _ = _batch()
    with torch.no_grad():
        a = model(idx)
        b = model(idx, doc_ids=torch.zeros_like(idx))
    torch.testing.assert_close(a, b, rtol=0.0, atol=1e-4)


def test_positions_are_clamped_to_the_table():
    """A document longer than n_positions must not index past wpe."""
    model = _model()  # n_positions = 64
    idx = torch.randint(0, 512, (1, 80))
    doc_ids = torch.zeros(1, 80, dtype=torch.int64)
    with torch.no_grad():
        assert torch.isfinite(model(idx, doc_ids=doc_ids)).all()


if __name__ == '__main__':
    sys.exit(pytest.main([__file__]))
