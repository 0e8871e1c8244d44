"""GPT-2 small training on synthetic tokens — the LLM fast path.

Demonstrates: bf16 flat replica (fp32 master in the fused optimizer),
fused LayerNorm + cross-entropy kernels, single-all-reduce gradient
sync, hipGraph-captured steps inside a TrainValStage.

Run:  python examples/gpt2.py
      torchrun --standalone --nproc-per-node 8 examples/gpt2.py
      python examples/gpt2.py --packed    # several documents per row
      python examples/gpt2.py --n-kv-head 4   # grouped-query attention

--packed fills every row with random-length documents that end in an EOS
token, keeps attention inside each document (ops.fused_attn: the native
kernels skip the tiles of other documents) and restarts the positions at
every document start. The last token of a document has no next token of
its own, so its target is the loss's ignore_index.

--n-kv-head gives K and V that many heads (a divisor of the model's
n_head; 1 is multi-query attention): the native kernels read the shared
K/V heads in place and sum each group's dK/dV in registers.
"""

import argparse
import sys

sys.path.insert(0, './')

import torch

from dmlcloud_amd import TrainingPipeline, TrainValStage
from dmlcloud_amd.models import gpt2_small, gpt2_tiny
from dmlcloud_amd.ops import document_starts_from_eos
from dmlcloud_amd.parallel import FlatAdamW, LRSchedule, init_process_group_auto, weight_decay_groups


class SyntheticTokens(torch.utils.data.Dataset):
    def __init__(self, n: int, seq_len: int, vocab: int, seed: int = 0):
        g = torch.Generator().manual_seed(seed)
        self.tokens = torch.randint(0, vocab, (n, seq_len), generator=g)

    def __len__(self):
        return len(self.tokens)

    def __getitem__(self, idx):
        return self.tokens[idx]


MAX_EPOCHS = 2
EOS_ID = 0
IGNORE_INDEX = -100  # ops.fused_loss.cross_entropy's default


class PackedSyntheticTokens(torch.utils.data.Dataset):
    """Rows of `seq_len` tokens, each a run of random-length documents
    (tokens 1..vocab-1) that end in EOS_ID; the last one is cut off by the
    end of the row, as a packing data loader would."""

    def __init__(self, n: int, seq_len: int, vocab: int, mean_len: int, seed: int = 0):
        g = torch.Generator().manual_seed(seed)
        self.tokens = torch.randint(1, vocab, (n, seq_len), generator=g)
        for row in self.tokens:
            end = -1
            while True:
                end += int(torch.randint(2, 2 * mean_len, (1,), generator=g))
                if end >= seq_len:
                    break
                row[end] = EOS_ID

    def __len__(self):
        return len(self.tokens)

    def __getitem__(self, idx):
        return self.tokens[idx]


def packed_targets(idx: torch.Tensor, doc_start: torch.Tensor) -> torch.Tensor:
    """Next-token targets that never cross a document: position i
    predicts token i + 1 unless i is the last token of its document (or of
    the row), which gets IGNORE_INDEX. No host sync."""
    targets = torch.full_like(idx, IGNORE_INDEX)
    same_doc = doc_start[:, 1:] == doc_start[:, :-1]
    targets[:, :-1] = torch.where(same_doc, idx[:, 1:], targets[:, :-1])
    return targets


class GPT2Stage(TrainValStage):
    def __init__(self, packed: bool = False, n_kv_head: int = None):
        super().__init__()
        self.packed = packed
        self.n_kv_head = n_kv_head

    def pre_stage(self):
        on_gpu = self.device.type == 'cuda'
        model = (gpt2_small if on_gpu else gpt2_tiny)(n_kv_head=self.n_kv_head)
        dtype = torch.bfloat16 if on_gpu else torch.float32
        self.pipeline.register_model('gpt2', model, ddp_impl='flat', flat_dtype=dtype)
        replica = self.pipeline.models['gpt2']
        vocab = replica.module.cfg.vocab_size
        seq = min(replica.module.cfg.n_positions, 1024)
        if self.packed:
            mean_len = max(seq // 5, 4)
            train = PackedSyntheticTokens(256, seq, vocab, mean_len)
            val = PackedSyntheticTokens(32, seq, vocab, mean_len, seed=1)
        else:
            train = SyntheticTokens(256, seq, vocab)
            val = SyntheticTokens(32, seq, vocab, seed=1)
        sampler = torch.utils.data.distributed.DistributedSampler(train)
        self.pipeline.register_dataset(
            'train', torch.utils.data.DataLoader(train, batch_size=8, sampler=sampler)
        )
        val_sampler = torch.utils.data.distributed.DistributedSampler(val, shuffle=False)
        self.pipeline.register_dataset(
            'val', torch.utils.data.DataLoader(val, batch_size=8, sampler=val_sampler)
        )

        # AdamW as GPT-2 is trained: matrices and embeddings decay, norm
        # gains and biases do not; linear warmup, then cosine decay to 10%.
        # The schedule runs on the device from the optimizer's own step
        # counter, so it also holds inside hipGraph-captured steps.
        total_steps = MAX_EPOCHS * len(self.pipeline.datasets['train'])
        schedule = LRSchedule.warmup_cosine(max(total_steps // 10, 1), total_steps, min_ratio=0.1)
        optimizer = FlatAdamW(
            replica, weight_decay_groups(model, 0.1), lr=3e-4, betas=(0.9, 0.95), schedule=schedule
        )
        self.pipeline.register_optimizer('adamw', optimizer)

    def step(self, batch):
        idx = batch.to(self.device)
        if self.packed:
            doc_ids = document_starts_from_eos(idx, EOS_ID)
            targets = packed_targets(idx, doc_ids)
            _, loss = self.pipeline.models['gpt2'](idx, targets=targets, doc_ids=doc_ids)
            return loss
        _, loss = self.pipeline.models['gpt2'](idx, targets=idx)
        return loss

    def gradient_clip(self):
        return 1.0


def main():
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    parser.add_argument('--packed', action='store_true', help='pack several documents into each row')
    parser.add_argument(
        '--n-kv-head', type=int, default=None, help='K/V heads for grouped-query attention (divides n_head)'
    )
    args = parser.parse_args()

    init_process_group_auto()
    pipeline = TrainingPipeline(name='gpt2-synthetic')
    pipeline.append_stage(GPT2Stage(packed=args.packed, n_kv_head=args.n_kv_head), max_epochs=MAX_EPOCHS)
    pipeline.run()


if __name__ == '__main__':
    main()
