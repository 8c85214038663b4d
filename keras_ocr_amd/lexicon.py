"""The caller's word list for lexicon-constrained recognition ("Lexicon"): strings -> label rows in the
recogniser's alphabet.  Pure host code; ``Recognizer.set_lexicon`` loads it into the context, where it stays like weights."""
import numpy as np

MAX_WORD = 32  # KOCR_LEXICON_MAX_WORD (include/kocr.h)
MAX_TOP = 64


def top_arg(lexicon_top):
    """``lexicon_top`` as an int, or ValueError naming the argument: 1 <= lexicon_top <= 64 (the library checks the same)."""
    k = int(lexicon_top)
    if not 1 <= k <= MAX_TOP:
        raise ValueError(f"lexicon_top {k} outside [1, {MAX_TOP}]")
    return k


class Lexicon:
    """``words``: an iterable of strings; ``alphabet``: the recogniser's (label c is ``alphabet[c]``, the blank is
    ``len(alphabet)``); ``lowercase``: lower-case every word first (the pretrained alphabet has no capitals).

    Duplicates (after lower-casing) are merged, the first occurrence kept: ``lexicon.words`` is the list the indices of a
    match refer to.  ``labels`` (V, width) int32, -1 padded, and ``lengths`` (V,) int32 are what ``Context.set_lexicon`` takes;
    ``classes`` = ``len(alphabet) + 1`` is the class count of the recogniser they are valid for.
    ValueError naming the word: an empty string, a character outside the alphabet, more than 32 characters."""

    def __init__(self, words, alphabet, lowercase=False):
        if isinstance(words, str):
            raise ValueError(f"a lexicon is a list of words, not the string {words!r}")
        self.alphabet = alphabet
        self.classes = len(alphabet) + 1
        code = {ch: i for i, ch in reversed(list(enumerate(alphabet)))}  # the first index of a repeated entry, as str.index
        self.words, rows, seen = [], [], set()
        for n, word in enumerate(words):
            if not isinstance(word, str):
                raise ValueError(f"lexicon word {n} is not a string: {word!r}")
            if lowercase:
                word = word.lower()
            if not word:
                raise ValueError(f"lexicon word {n} is the empty string {word!r}")
            if len(word) > MAX_WORD:
                raise ValueError(f"lexicon word {n}, {word!r}, has {len(word)} characters: more than {MAX_WORD}")
            bad = [ch for ch in word if ch not in code]
            if bad:
                raise ValueError(f"lexicon word {n}, {word!r}, has the character {bad[0]!r} outside the alphabet")
            if word in seen:
                continue
            seen.add(word)
            self.words.append(word)
            rows.append([code[ch] for ch in word])
        width = max([1] + [len(r) for r in rows])
        self.labels = np.full((len(rows), width), -1, np.int32)
        for v, row in enumerate(rows):
            self.labels[v, :len(row)] = row
        self.lengths = np.array([len(r) for r in rows], np.int32)

    def __len__(self):
        return len(self.words)
