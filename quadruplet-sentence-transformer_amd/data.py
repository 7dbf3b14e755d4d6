"""Batch construction for the real-text fit() driver.

The fused quadruplet pass pads all 4*B sequences of a batch to the longest one (rounded up to a multiple of 32), so a
batch costs 4 * B * L_max tokens of encoder work whatever the other lengths are. LengthBucketBatchSampler groups
examples of similar length: the reference's `DataLoader(dataset, shuffle=True, batch_size=B)`
(/root/reference/training/main.py:42-44) becomes `DataLoader(dataset, batch_sampler=LengthBucketBatchSampler(...))`,
with fit() and smart_batching_collate unchanged."""
from __future__ import annotations

import gzip
import random
from typing import Iterator, List, Sequence

import numpy as np
from torch.utils.data import Dataset, IterableDataset

from .sentence_transformer import InputExample


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


class ParallelSentencesDataset(Dataset):
    """sentence-transformers 2.2.2's `datasets.ParallelSentencesDataset`, the data side of losses.MSELoss: parallel sentences
    (a source sentence and its translations, or just the sentence itself for a plain distillation) become
    `InputExample(texts=[sentence], label=teacher embedding of the SOURCE sentence)` -- one example for the source and one
    for every translation, so that the student learns to put all of them where the teacher puts the source.

    Several datasets can be added (`load_data` from a tab-separated file, `.gz` accepted, one source sentence followed by
    its translations per line; `add_dataset` from lists). `generate_data` takes one entry from a dataset `weight` times for
    every dataset -- so the datasets are drawn in proportion to their weights --, has the teacher encode the source
    sentences in batches of `batch_size` (`teacher_model` is any object with `encode()`; with `use_embedding_cache` a
    sentence is encoded once and its embedding kept), and shuffles the resulting examples; `__getitem__` hands them out
    and generates the next round when they run out, whatever index is asked for. `len()` is the number of sentences
    (sources and translations) of all datasets. A dataset is walked through in order and reshuffled when it has been
    exhausted. Feed it through `DataLoader(dataset, shuffle=False, batch_size=...)` and fit()'s collate function.

    `student_model` is kept for the signature's sake and not used, as in 2.2.2. Where this differs from 2.2.2: the
    translations of a source keep the order in which they were first seen (2.2.2 holds them in a set, whose order changes
    from process to process); shuffling uses the `random` module's global generator, as there."""

    def __init__(self, student_model, teacher_model, batch_size: int = 8, use_embedding_cache: bool = True):
        self.student_model = student_model
        self.teacher_model = teacher_model
        self.batch_size = batch_size
        self.use_embedding_cache = use_embedding_cache
        self.datasets = []                # per dataset: [(source, [source and its translations])]
        self.datasets_iterator = []       # per dataset: the next entry to take
        self.dataset_indices = []         # dataset ids, each `weight` times: one round of generate_data
        self.cache = []                   # the examples of the current round
        self.embedding_cache = {}
        self.num_sentences = 0

    @staticmethod
    def _too_long(sentences, max_sentence_length) -> bool:
        return max_sentence_length is not None and max_sentence_length > 0 and \
            max(len(sent) for sent in sentences) > max_sentence_length

    def load_data(self, filepath: str, weight: int = 100, max_sentences: int = None, max_sentence_length: int = 128):
        """One line = the source sentence and its translations, separated by tabs. Lines with a sentence of more than
        max_sentence_length characters are passed over; reading stops after max_sentences kept lines."""
        parallel_sentences = []
        opener = gzip.open if filepath.endswith(".gz") else open
        with opener(filepath, "rt", encoding="utf8") as f:
            for line in f:
                sentences = line.strip().split("\t")
                if self._too_long(sentences, max_sentence_length):
                    continue
                parallel_sentences.append(sentences)
                if max_sentences is not None and 0 < max_sentences <= len(parallel_sentences):
                    break
        self.add_dataset(parallel_sentences, weight=weight, max_sentences=max_sentences,
                         max_sentence_length=max_sentence_length)

    def add_dataset(self, parallel_sentences: List[List[str]], weight: int = 100, max_sentences: int = None,
                    max_sentence_length: int = 128):
        """parallel_sentences: [[source, translation, ...], ...]. Entries with the same source are merged; at most
        max_sentences different sources are kept."""
        sentences_map = {}
        for sentences in parallel_sentences:
            if self._too_long(sentences, max_sentence_length):
                continue
            targets = sentences_map.setdefault(sentences[0], {})
            for sent in sentences:
                targets[sent] = None
            if max_sentences is not None and 0 < max_sentences <= len(sentences_map):
                break
        if not sentences_map:
            return
        self.num_sentences += sum(len(t) for t in sentences_map.values())
        dataset_id = len(self.datasets)
        self.datasets.append([(src, list(t)) for src, t in sentences_map.items()])
        self.datasets_iterator.append(0)
        self.dataset_indices.extend([dataset_id] * weight)

    def next_entry(self, data_idx: int):
        source, targets = self.datasets[data_idx][self.datasets_iterator[data_idx]]
        self.datasets_iterator[data_idx] += 1
        if self.datasets_iterator[data_idx] >= len(self.datasets[data_idx]):
            self.datasets_iterator[data_idx] = 0
            random.shuffle(self.datasets[data_idx])
        return source, targets

    def generate_data(self):
        entries = [self.next_entry(data_idx) for data_idx in self.dataset_indices]
        src_embeddings = self.get_embeddings([src for src, _ in entries])
        for src_embedding, (_, targets) in zip(src_embeddings, entries):
            for sent in targets:
                self.cache.append(InputExample(texts=[sent], label=src_embedding))
        random.shuffle(self.cache)

    def get_embeddings(self, sentences: List[str]):
        """The teacher's embeddings of `sentences`, in their order."""
        encode = lambda xs: self.teacher_model.encode(xs, batch_size=self.batch_size, show_progress_bar=False,  # noqa: E731
                                                      convert_to_numpy=True)
        if not self.use_embedding_cache:
            return encode(sentences)
        new_sentences = list(dict.fromkeys(s for s in sentences if s not in self.embedding_cache))
        if new_sentences:
            for sent, embedding in zip(new_sentences, encode(new_sentences)):
                self.embedding_cache[sent] = embedding
        return [self.embedding_cache[sent] for sent in sentences]

    def __len__(self) -> int:
        return self.num_sentences

    def __getitem__(self, idx):
        if not self.cache:
            self.generate_data()
        return self.cache.pop()
