"""What follows detection and recognition: the words of a page grouped into text lines, in reading order, on the GPU
(kocr_group_lines; DESIGN.md section 4, "Lines"), the lines cut into blocks -- columns and paragraphs -- in reading order
(the same call with KOCR_LINES_BLOCKS; "Blocks"), the words of a table put into rows, columns and spanning cells (the same call
with KOCR_LINES_TABLE; "Tables"), and the type of a word's character boxes (kocr_char_boxes; "Characters").  The reference has no counterpart -- its ``tools.combine_line`` / ``fix_line`` serve training
labels that are already grouped -- and there is no host path."""
import math
import typing

import numpy as np

from . import _lib


class Line(typing.NamedTuple):
    """One text line of a page: ``box`` (4, 2) float32, the bounding rectangle along the line's axis [tl, tr, br, bl];
    ``words``: the indices of its words in the page's list of boxes, in reading order."""
    box: np.ndarray
    words: typing.List[int]


class Block(typing.NamedTuple):
    """One block of a page (a column, a paragraph, a heading): ``box`` (4, 2) float32, the box [tl, tr, br, bl] around its
    members -- axis-aligned from ``group_blocks``, a rectangle along the page's text direction from
    ``group_blocks_deskewed``; ``lines``: the indices of its members in the page's list of boxes, top to bottom."""
    box: np.ndarray
    lines: typing.List[int]


class Cell(typing.NamedTuple):
    """One cell of a table: the words of one ``row`` that start in column ``col``; it reaches over ``colspan`` columns
    (more than 1: a spanning cell, such as a title row or a merged header).  ``words``: from ``group_table`` the indices
    of its words in the page's list of boxes, from ``Pipeline.recognize_table`` recognize()'s own ``(text, box)`` tuples,
    either way from left to right; ``text``: their texts joined by single spaces (None from ``group_table``, which sees
    no text)."""
    row: int
    col: int
    colspan: int
    words: list
    text: typing.Optional[str] = None


class Table(typing.NamedTuple):
    """The words of one table as a grid ("Tables"): ``rows`` and ``cols``, its size; ``row_boxes``
    (rows, 4, 2) and ``col_boxes`` (cols, 4, 2) float32, the bands [tl, tr, br, bl] of every row (the table's width, the
    row's height) and every column (between two separators, the table's height); ``cells``: the ``Cell``s that hold words,
    in reading order -- row after row, left to right inside a row.  A page without words is a table of 0 x 0."""
    rows: int
    cols: int
    row_boxes: np.ndarray
    col_boxes: np.ndarray
    cells: typing.List[Cell]

    def grid(self):
        """``rows`` lists of ``cols`` strings: every cell's ``text`` at (row, col) -- a spanning cell's at its first column
        --, ``""`` where no word starts.  Cells without text (``group_table``) show their word indices joined by spaces."""
        out = [[""] * self.cols for _ in range(self.rows)]
        for cell in self.cells:
            out[cell.row][cell.col] = cell.text if cell.text is not None else " ".join(str(w) for w in cell.words)
        return out


class Characters(typing.NamedTuple):
    """The characters of one word box, read off the detector's region map ("Characters"): ``boxes``
    (K, 4, 2) float32, one quad [tl, tr, br, bl] per character from the word's tl towards its tr, each a slice of the word
    box at its full height; ``scores`` (K,) float32, the region map's value at each character's peak.  K counts the blobs
    of the region map, not the letters the recogniser read: the two need not agree."""
    boxes: np.ndarray
    scores: np.ndarray


class Orientation(typing.NamedTuple):
    """How one word was read ("Orientation"): ``turns``, the quarter turns of the better of the two
    readings (0 as detected, 1 text running down the page, 2 upside down, 3 up the page); ``box`` (4, 2) float32, the word's
    box [tl, tr, br, bl] of the text AS READ -- ``box[0] -> box[1]`` is the reading direction; ``log_words``, the exact CTC
    log-probabilities ``(v_0, v_1)`` of the two candidates' own decodes (turns ``t`` and ``t + 2`` of the fewer-turns
    candidate), so that a caller sees the margin of the choice."""
    turns: int
    box: np.ndarray
    log_words: typing.Tuple[float, float]


def orientations_of(turns, quads, log_words):
    """``Context.recognition_orientation``'s arrays as one ``Orientation`` per word"""
    return [Orientation(int(t), q, (float(v[0]), float(v[1]))) for t, q, v in zip(np.asarray(turns).tolist(), quads, np.asarray(log_words))]


def characters_of(char_groups):
    """``Context.char_boxes``' per-image lists of ``(quads, scores)`` pairs as lists of ``Characters``"""
    return [[Characters(quads, scores) for quads, scores in page] for page in char_groups]


def _context(ctx):
    return _lib.default_context() if ctx is None or ctx is True else ctx


def _groups(record, offsets, group_of, order, group_counts, boxes):
    """kocr_group_lines' arrays as, per page, a list of ``record(box, members)``: ``order`` lists a page's members group
    after group, ``group_of`` says how many each group has"""
    pages, group = [], 0
    for i, groups in enumerate(group_counts.tolist()):
        members = order[offsets[i]:offsets[i + 1]].tolist()
        page, at = [], 0
        lengths = np.bincount(group_of[offsets[i]:offsets[i + 1]], minlength=groups).tolist() if groups else []
        for k in range(groups):
            page.append(record(boxes[group + k], members[at:at + lengths[k]]))
            at += lengths[k]
        pages.append(page)
        group += groups
    return pages


def group_lines(box_groups, ctx=None, **rule):
    """Per image the text lines of its word boxes: ``box_groups`` is a list (one entry per image) of (n_i, 4, 2) boxes
    [tl, tr, br, bl], e.g. ``Detector.detect``'s result or the boxes of ``Pipeline.recognize``.  Returns, per image, a list
    of ``Line(box, words)`` from the top of the page to its bottom.  One GPU call for the whole batch; ``ctx`` is a
    ``Context`` (None or True: the default one).  ``rule``: ``max_angle`` (degrees, default 15), ``min_height_ratio`` (0.5),
    ``max_offset`` (0.5), ``max_gap`` (1.5) -- when two words belong to one line, see ``Context.group_lines``.  The defaults
    are judgement, not fitted to real pages.  Columns are not detected: two columns side by side interleave -- hand the
    line boxes to ``group_blocks`` for a column-aware reading order.  At most 2048 words per image (ValueError)."""
    unknown = set(rule) - {"max_angle", "min_height_ratio", "max_offset", "max_gap"}
    if unknown:
        raise TypeError(f"group_lines: unknown rule parameter(s) {sorted(unknown)}")
    counts, quads = _lib._flatten_boxes(box_groups)  # pylint: disable=protected-access
    offsets = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int32)
    return _groups(Line, offsets, *_context(ctx).group_lines(quads, offsets, **rule))


def group_blocks(box_groups, ctx=None, min_gap_x=1.0, min_gap_y=0.75):
    """Per image its boxes cut into blocks -- columns, paragraphs, headings -- in reading order, by a recursive XY-cut on the
    GPU (kocr_group_lines with KOCR_LINES_BLOCKS; DESIGN.md section 4, "Blocks").  ``box_groups`` is a list (one entry per
    image) of (n_i, 4, 2) boxes, in practice the line boxes of ``group_lines``.  Returns, per image, a list of
    ``Block(box, lines)`` in reading order, ``lines`` the indices into that image's boxes from the top of the block to its
    bottom.  One GPU call for the whole batch; ``ctx`` as in ``group_lines``.  ``min_gap_x`` / ``min_gap_y``: the narrowest
    gutter and the smallest paragraph gap that are cut, in mean line heights -- see ``Context.group_blocks``; the defaults
    are judgement, not fitted to real pages.  The cut is axis-aligned (``group_blocks_deskewed`` takes a rotated page) and whitespace is its
    only cue: a paragraph gap wider than the heading's and the footer's is cut before them.  At most 2048 boxes per image
    (ValueError)."""
    counts, quads = _lib._flatten_boxes(box_groups)  # pylint: disable=protected-access
    offsets = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int32)
    return _groups(Block, offsets, *_context(ctx).group_blocks(quads, offsets, min_gap_x=min_gap_x, min_gap_y=min_gap_y))


def group_blocks_deskewed(box_groups, ctx=None, min_gap_x=1.0, min_gap_y=0.75):
    """``group_blocks`` for rotated pages -- a skewed scan, a photo, a page fed in sideways or upside down (kocr_group_lines
    with KOCR_LINES_BLOCKS | KOCR_LINES_DESKEW; DESIGN.md section 4, "Rotated pages").  Every image's text direction is
    estimated on the GPU from its own boxes (the weighted medoid of their tl -> tr directions), the XY-cut runs in that
    frame, and ``Block.box`` is a rotated rectangle in page coordinates whose tl -> tr runs along the text: ``box_angle``
    reads the page's skew off any of them.  Arguments, return value and limits are ``group_blocks``', and on a page that is
    not rotated so are the numbers.  Not covered: a page whose text runs in several directions, and a page turned by 90 or
    180 degrees whose boxes were not read with ``orientation`` (tl -> tr is then not the reading direction)."""
    counts, quads = _lib._flatten_boxes(box_groups)  # pylint: disable=protected-access
    offsets = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int32)
    return _groups(Block, offsets, *_context(ctx).group_blocks_deskewed(quads, offsets, min_gap_x=min_gap_x, min_gap_y=min_gap_y))


def group_table(box_groups, ctx=None, **rule):
    """Per image its word boxes as a table: rows, columns and spanning cells, by the white space between the boxes, on the
    GPU (kocr_group_lines with KOCR_LINES_TABLE; DESIGN.md section 4, "Tables").  ``box_groups`` is a list (one entry per
    image) of (n_i, 4, 2) boxes: the words of ONE table each -- a whole page, or the words of one ``Block``.  Returns, per
    image, a ``Table``.  One GPU call for the whole batch; ``ctx`` as in ``group_lines``.  ``rule``: ``min_gap_x`` (1.0:
    the narrowest column gutter, in mean word heights), ``min_gap_y`` (0.25: the smallest leading that separates two
    rows), ``min_support`` (0.5: the share of the rows that must show a gutter) -- see ``Context.group_table``; the
    defaults are judgement, not fitted to real pages.  The rule is axis-aligned, whitespace is its only cue (no ruling
    lines), and a cell whose text wraps becomes two rows unless ``min_gap_y`` is raised.  At most 2048 boxes per image
    (ValueError)."""
    unknown = set(rule) - {"min_gap_x", "min_gap_y", "min_support"}
    if unknown:
        raise TypeError(f"group_table: unknown rule parameter(s) {sorted(unknown)}")
    counts, quads = _lib._flatten_boxes(box_groups)  # pylint: disable=protected-access
    offsets = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int32)
    row_of, col_first, col_last, row_counts, col_counts, row_boxes, col_boxes = _context(ctx).group_table(quads, offsets, **rule)
    left = np.asarray(quads, dtype=np.float32).reshape(-1, 4, 2)[:, :, 0].min(axis=1)
    tables, row_at, col_at = [], 0, 0
    for i, (rows, cols) in enumerate(zip(np.asarray(row_counts).tolist(), np.asarray(col_counts).tolist())):
        a, b = int(offsets[i]), int(offsets[i + 1])
        keys = zip(row_of[a:b].tolist(), col_first[a:b].tolist(), left[a:b].tolist(), range(b - a), col_last[a:b].tolist())
        cells = {}  # (row, col) -> [last column, words]; filled in reading order, which a dict keeps
        for row, col, _, j, last in sorted(keys):
            cell = cells.setdefault((row, col), [last, []])
            cell[0] = max(cell[0], last)
            cell[1].append(j)
        tables.append(Table(rows, cols, row_boxes[row_at:row_at + rows], col_boxes[col_at:col_at + cols],
                            [Cell(row, col, last - col + 1, words) for (row, col), (last, words) in cells.items()]))
        row_at, col_at = row_at + rows, col_at + cols
    return tables


def box_angle(box):
    """The direction of ``box``'s tl -> tr in degrees, in (-180, 180], by atan2 (y grows down the page: a positive angle is a
    clockwise turn on screen); 0.0 for a box without width.  How a caller reads a page's skew off any block box of
    ``group_blocks_deskewed``.  For display only: nothing on the device uses an angle."""
    b = np.asarray(box, dtype=np.float64).reshape(4, 2)
    dx, dy = float(b[1, 0] - b[0, 0]), float(b[1, 1] - b[0, 1])
    if dx == 0 and dy == 0:
        return 0.0
    angle = math.degrees(math.atan2(dy, dx))
    return 180.0 if angle == -180.0 else angle
