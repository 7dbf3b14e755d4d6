"""Batch construction for the real-text fit() driver.

The fused quadruplet pass pads all 4*B sequences of a batch to the longest one (rounded up to a multiple of 32), so a
batch costs 4 * B * L_max tokens of encoder work whatever the other lengths are. LengthBucketBatchSampler groups
examples of similar length: the reference's `DataLoader(dataset, shuffle=True, batch_size=B)`
(/root/reference/training/main.py:42-44) becomes `DataLoader(dataset, batch_sampler=LengthBucketBatchSampler(...))`,
with fit() and smart_batching_collate unchanged."""
from __future__ import annotations

import random
from typing import Iterator, List, Sequence

import numpy as np
from torch.utils.data import IterableDataset


class LengthBucketBatchSampler:
    """Yields lists of dataset indices. Every epoch: shuffle, cut into pools of `pool_batches` batches, sort each pool by
    length, cut it into batches, then shuffle the order of all batches -- batches hold examples of similar length while
    their composition and order still change from epoch to epoch (a full sort would fix both).

    lengths: tokens per example (SentenceTransformer.token_lengths). drop_last as torch's BatchSampler."""

    def __init__(self, lengths: Sequence[int], batch_size: int, shuffle: bool = True, seed: int = 14, pool_batches: int = 50,
                 drop_last: bool = False):
        if batch_size <= 0 or pool_batches <= 0:
            raise ValueError("batch_size and pool_batches must be positive")
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.batch_size, self.shuffle, self.seed = int(batch_size), bool(shuffle), int(seed)
        self.pool_batches, self.drop_last = int(pool_batches), bool(drop_last)
        self.epoch = 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __len__(self) -> int:
        n = len(self.lengths)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self) -> Iterator[List[int]]:
        n = len(self.lengths)
        rng = np.random.default_rng(self.seed + self.epoch)
        order = rng.permutation(n) if self.shuffle else np.arange(n)
        pool = self.batch_size * self.pool_batches
        batches = []
        for p0 in range(0, n, pool):
            idx = order[p0:p0 + pool]
            idx = idx[np.argsort(self.lengths[idx], kind="stable")]
            for b0 in range(0, len(idx), self.batch_size):
                b = idx[b0:b0 + self.batch_size]
                if len(b) == self.batch_size or not self.drop_last:
                    batches.append(b.tolist())
        if self.shuffle:
            batches = [batches[i] for i in rng.permutation(len(batches))]
        self.epoch += 1
        return iter(batches)


def padded_tokens(lengths: Sequence[int], batches: Sequence[Sequence[int]], multiple: int = 32) -> int:
    """Encoder token rows a list of batches costs: per batch, size x the longest example rounded up to `multiple`."""
    L = np.asarray(lengths)
    return int(sum(len(b) * (-(-int(L[list(b)].max()) // multiple) * multiple) for b in batches if len(b)))


class NoDuplicatesDataLoader:
    """sentence-transformers 2.2.2's `datasets.NoDuplicatesDataLoader`: batches of `batch_size` examples in which no text
    appears twice (compared stripped and lower-cased, over every text column), as the in-batch-negatives losses need -- a
    text that is the positive of one anchor and sits in the batch a second time would be scored as a negative of itself.

    The examples are shuffled in place once, then walked with a pointer that persists across epochs: an example whose texts
    collide with the batch being filled is passed over for this batch (it comes round again on the next lap), and at the
    end of the list the pointer wraps to the start after a reshuffle. `len()` is floor(len(examples) / batch_size);
    `collate_fn` is an attribute fit() sets. Where sentence-transformers would spin for ever -- fewer distinct examples
    than one batch needs -- a lap that adds nothing raises ValueError."""

    def __init__(self, train_examples, batch_size: int):
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        self.batch_size = int(batch_size)
        self.data_pointer = 0
        self.collate_fn = None
        self.train_examples = train_examples
        random.shuffle(self.train_examples)

    def __len__(self) -> int:
        return len(self.train_examples) // self.batch_size

    def __iter__(self):
        n = len(self.train_examples)
        for _ in range(len(self)):
            batch, seen, idle = [], set(), 0
            while len(batch) < self.batch_size:
                example = self.train_examples[self.data_pointer]
                keys = [t.strip().lower() for t in example.texts]
                if not any(k in seen for k in keys):
                    batch.append(example)
                    seen.update(keys)
                    idle = 0
                else:
                    idle += 1
                    if idle > n:
                        raise ValueError(f"NoDuplicatesDataLoader: no {self.batch_size} examples without a repeated text")
                self.data_pointer += 1
                if self.data_pointer >= n:
                    self.data_pointer = 0
                    random.shuffle(self.train_examples)
            yield self.collate_fn(batch) if self.collate_fn is not None else batch


class SentenceLabelDataset(IterableDataset):
    """sentence-transformers 2.2.2's `datasets.SentenceLabelDataset`: the examples (one text, one integer label each) in
    runs of `samples_per_label` consecutive examples of one label, so that every batch cut from the stream --
    `DataLoader(SentenceLabelDataset(examples), batch_size=...)`, batch_size a multiple of samples_per_label -- holds
    positives for the batch-mining triplet losses.

    Labels with fewer than `samples_per_label` examples are dropped; `len()` is the number of examples kept. One pass
    yields whole runs until `len()` examples have gone out (the last run is not cut short). The labels are visited in a
    shuffled order; within a lap an example is not drawn twice unless `with_replacement`; a label with too few unseen
    examples left is passed over, and when the labels are exhausted the order is reshuffled and every example is unseen
    again. Draws come from numpy's global generator."""

    def __init__(self, examples, samples_per_label: int = 2, with_replacement: bool = False):
        super().__init__()
        if samples_per_label < 1:
            raise ValueError("samples_per_label must be positive")
        self.samples_per_label = int(samples_per_label)
        self.with_replacement = bool(with_replacement)
        by_label = {}
        for example in examples:
            by_label.setdefault(example.label, []).append(example)
        self.grouped_inputs, self.groups_right_border = [], []      # the kept examples label by label; where each group ends
        for group in by_label.values():
            if len(group) >= self.samples_per_label:
                self.grouped_inputs.extend(group)
                self.groups_right_border.append(len(self.grouped_inputs))
        self.label_range = np.arange(len(self.groups_right_border))
        np.random.shuffle(self.label_range)

    def __len__(self) -> int:
        return len(self.grouped_inputs)

    def __iter__(self):
        n_labels = len(self.label_range)
        at, count, seen = 0, 0, {}
        while count < len(self.grouped_inputs):
            group = int(self.label_range[at])
            lo = self.groups_right_border[group - 1] if group > 0 else 0
            mine = seen.setdefault(group, set())
            pool = [i for i in range(lo, self.groups_right_border[group]) if self.with_replacement or i not in mine]
            if len(pool) >= self.samples_per_label:
                for i in np.random.choice(pool, self.samples_per_label, replace=False):
                    count += 1
                    mine.add(int(i))
                    yield self.grouped_inputs[int(i)]
            at += 1
            if at >= n_labels:
                at, seen = 0, {}
                np.random.shuffle(self.label_range)
