"""Character sets ("Character sets"): named subsets of a recogniser's alphabet that a crop may be
decoded under -- "digits", "upper-case codes" -- as the table ``Context.set_charsets`` loads."""
import numpy as np

MAX_SETS = 256  # include/kocr.h: KOCR_CHARSETS_MAX


def table(charsets, alphabet, lowercase=False):
    """``charsets``: a mapping name -> characters (a string or an iterable of one-character strings); ``alphabet``: the
    recogniser's (class c is ``alphabet[c]``; the blank, ``len(alphabet)``, is always allowed and has no column);
    ``lowercase``: lower-case the characters first (the pretrained alphabet has no capitals).  Returns ``(names, allowed)``:
    the names in the mapping's order and a (S, len(alphabet)) uint8 table, row s the classes of set ``names[s]``.

    ValueError naming the set and the character for one outside the alphabet; for an empty set, for no or more than 256
    sets, and for something that is not a mapping of names to characters."""
    if not hasattr(charsets, "items"):
        raise ValueError(f"charsets must be a mapping name -> characters, got {type(charsets).__name__}")
    if not 1 <= len(charsets) <= MAX_SETS:
        raise ValueError(f"{len(charsets)} character sets: there must be between 1 and {MAX_SETS}")
    code = {ch: c for c, ch in enumerate(alphabet)}
    names, allowed = [], np.zeros((len(charsets), len(alphabet)), np.uint8)
    for s, (name, chars) in enumerate(charsets.items()):
        if not isinstance(name, str):
            raise ValueError(f"character set {s} has the name {name!r}: names are strings")
        chars = list(chars)
        if any(not isinstance(ch, str) for ch in chars):
            raise ValueError(f"character set {name!r} must hold characters, got {chars!r}")
        if lowercase:
            chars = [ch.lower() for ch in chars]
        if not chars:
            raise ValueError(f"character set {name!r} is empty: a set needs at least one character")
        for ch in chars:
            if ch not in code:
                raise ValueError(f"character set {name!r} has the character {ch!r} outside the alphabet")
            allowed[s, code[ch]] = 1
        names.append(name)
    return names, allowed


def index_of(names, charset):
    """The index of the set called ``charset`` among the loaded ``names`` (None stays None: no set); ValueError listing the
    loaded names for an unknown one."""
    if charset is None:
        return None
    if not isinstance(charset, str) or charset not in (names or []):
        raise ValueError(f"unknown character set {charset!r}: the loaded sets are {list(names or [])} (Recognizer.set_charsets)")
    return names.index(charset)


def per_box(names, charset, box_groups):
    """``charset`` for ``recognize_from_boxes``: None -> (None, None); a name -> (its index, None): one set for every box;
    per-image lists of per-box name-or-None -> (None, the flat list of indices, -1 for None).  ValueError for an unknown
    name and for lists that do not match ``box_groups``."""
    if charset is None or isinstance(charset, str):
        return index_of(names, charset), None
    groups = list(charset)
    if len(groups) != len(box_groups):
        raise ValueError(f"charset: {len(groups)} per-image lists for {len(box_groups)} box groups")
    flat = []
    for i, (sets, boxes) in enumerate(zip(groups, box_groups)):
        sets = [sets] * len(boxes) if sets is None or isinstance(sets, str) else list(sets)
        if len(sets) != len(boxes):
            raise ValueError(f"charset: image {i} has {len(sets)} entries for {len(boxes)} boxes")
        flat.extend(-1 if name is None else index_of(names, name) for name in sets)
    return None, np.asarray(flat, np.int32)
