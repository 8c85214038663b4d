"""Host-side mirror of ``keras_ocr.pipeline.Pipeline`` (reference ``keras_ocr/pipeline.py:7-75``)."""
import numpy as np

from . import _lib, detection, evaluation as _evaluation, layout as _layout, recognition, scores as _scores, tools
from .extras import Extras, only_uint8
from .results import Results, decode_labels  # noqa: F401  (decode_labels: imported from here by callers)


def beam_of(recognition_kwargs):
    """``(beam_width, top_paths)`` from recognize()'s ``recognition_kwargs``, validated (ValueError naming the argument), or None"""
    return Extras.asked(recognition_kwargs).checked_beam()


def lexicon_of(recognition_kwargs):
    """``lexicon_top`` from ``recognition_kwargs``, validated (ValueError also together with ``beam_width``), or None"""
    return Extras.asked(recognition_kwargs).checked_lexicon_top()


def orientation_of(recognition_kwargs, char_boxes=None):
    """``(orientation, tall_ratio)`` from ``recognition_kwargs``, validated (ValueError naming the argument, or naming both
    when it is combined with ``beam_width``, ``lexicon_top`` or character boxes), or None"""
    return Extras.asked(recognition_kwargs, char_boxes=char_boxes).checked_orientation()


def label_width_of(recognizer):
    """The width of ``recognizer``'s label rows: its libkocr context's ``crnn_label_width()`` (50 - rnn_steps_to_discard; 48 by
    default), else its ``label_width`` attribute (a duck-typed recogniser may define one), else None: it reports no width."""
    ctx = getattr(recognizer, "_ctx", None)
    if ctx is not None and hasattr(ctx, "crnn_label_width"):
        return int(ctx.crnn_label_width())
    width = getattr(recognizer, "label_width", None)
    return None if width is None else int(width)


class Pipeline:
    """A wrapper for a combination of detector and recognizer (pipeline.py:7-26).

    Args:
        detector: The detector to use
        recognizer: The recognizer to use
        scale: The scale factor to apply to input images
        max_size: The maximum single-side dimension of images for inference.
    """

    def __init__(self, detector=None, recognizer=None, scale=2, max_size=2048):
        if detector is None:
            detector = detection.Detector()
        if recognizer is None:
            recognizer = recognition.Recognizer()
        self.scale = scale
        self.detector = detector
        self.recognizer = recognizer
        self.max_size = max_size

    def _plan(self, shapes):
        """resize_image's scale rule per image + the batch's padded size (pipeline.py:44-57)."""
        scales = [tools.resize_scale(s, self.scale, self.max_size) for s in shapes]
        dws = [int(s[1] * sc) for s, sc in zip(shapes, scales)]
        dhs = [int(s[0] * sc) for s, sc in zip(shapes, scales)]
        return scales, dhs, dws, max(dhs), max(dws)

    def recognize(self, images, detection_kwargs=None, recognition_kwargs=None):
        """Pipeline.recognize (pipeline.py:28-75): list of images (arrays or file paths) or an
        (N,H,W,3) array -> list (per image) of (text, box) tuples, boxes in input-image pixels.

        ``recognition_kwargs={"beam_width": B, "top_paths": K}`` ("Beam search"): every ``text`` becomes
        a list of up to K alternatives ``(text, log_prob)``, best first, as ``Recognizer.recognize``; the boxes are the same
        bits.  ``recognition_kwargs={"lexicon_top": K}`` (section 4, "Lexicon"; after ``recognizer.set_lexicon(words)``): every
        ``text`` becomes a list of up to K ``(word, log_prob)`` lexicon matches, best first.  Not both (ValueError).  The other
        keys of both dicts are Keras predict arguments without effect.

        ``recognition_kwargs={"orientation": "flip" | "any", "tall_ratio": r}`` (section 4, "Orientation"): every box is read
        in two orientations on the GPU and the better reading kept, as ``Recognizer.recognize_from_boxes``; each ``text`` is
        the winner's and each ``box`` the word's box [tl, tr, br, bl] of the text as read (the detector's rectangle, its corners
        renamed), so ``box[0] -> box[1]`` is the reading direction.  Not together with ``beam_width``, ``lexicon_top`` or
        character boxes (ValueError); uint8 images only (NotImplementedError).  ``recognize_with_scores``, ``recognize_lines``,
        ``evaluate``, ``recognize_padded`` and ``recognize_raw`` take it in the same way.

        ``recognition_kwargs={"charset": name}`` (section 4, "Character sets"; after
        ``recognizer.set_charsets({name: characters})``): every box is decoded under that set, whatever else is asked for;
        the boxes are the same bits.  ValueError listing the loaded names for an unknown one.

        ``recognition_kwargs={"pattern": name}`` (section 4, "Patterns"; after ``recognizer.set_patterns({name: regex})``):
        every ``text`` becomes ``(text, log_prob)``, the best reading of the box that the regular expression accepts and its
        exact CTC log-probability, ``(None, -inf)`` where nothing fits; the boxes are the same bits.  Not together with
        ``beam_width``, ``lexicon_top``, ``charset`` or ``orientation`` (ValueError); uint8 images only (NotImplementedError).
        ``recognize_with_scores``, ``recognize_padded``, ``recognize_raw`` and ``recognize_tiled`` take it in the same way."""
        return self.recognize_padded(images, None, None, detection_kwargs, recognition_kwargs)

    def recognize_with_scores(self, images, detection_kwargs=None, recognition_kwargs=None):
        """recognize() that also says how sure the two networks were: (text, box, score) tuples, ``score`` a
        ``scores.Score`` (detection, word, log_word, characters), computed on the GPU in the same pass (DESIGN.md section 4,
        "Scores").  Texts and boxes are recognize()'s, bit for bit.  A method of its own because recognize() keeps the
        reference's exact signature; ``recognize_padded`` / ``recognize_device`` take ``return_scores=True`` instead.
        With a ``beam_width`` in ``recognition_kwargs`` the tuples are (alternatives, box, score); ``score.word`` /
        ``log_word`` / ``characters`` keep referring to the greedy decode, which need not be the first alternative."""
        return self.recognize_padded(images, None, None, detection_kwargs, recognition_kwargs, return_scores=True)

    def evaluate(self, images, true, detection_kwargs=None, recognition_kwargs=None, **score_kwargs):
        """recognize() scored against labelled pages on the GPU (evaluation.score with the detector's context; DESIGN.md
        section 4, "Evaluation").  ``true``: one list of annotations ``{"text", "vertices"[, "ignore"]}`` per image;
        ``score_kwargs``: ``iou_threshold``, ``similarity_threshold``, ``translator``, ``return_results``.  Returns
        ``(predictions, results, (precision, recall))``: ``predictions`` is what recognize() returns, ``results`` and the two
        numbers what ``evaluation.score({i: true[i]}, {i: [{"text", "vertices"} per word]})`` returns, the image ids being
        the positions in ``images``.  ``beam_width`` / ``lexicon_top`` are refused (ValueError): their ``text`` is a list."""
        Extras.asked(recognition_kwargs).one_text_per_word("evaluate scores one text per word")
        true = list(true)
        predictions = self.recognize(images, detection_kwargs, recognition_kwargs)
        if len(true) != len(predictions):
            raise ValueError(f"{len(predictions)} images but {len(true)} lists of annotations")
        pred = {i: [{"text": text, "vertices": box} for text, box in group] for i, group in enumerate(predictions)}
        ctx = getattr(self.detector, "_ctx", None)
        results, precision_recall = _evaluation.score(dict(enumerate(true)), pred, ctx=True if ctx is None else ctx, **score_kwargs)
        return predictions, results, precision_recall

    def recognize_lines(self, images, detection_kwargs=None, recognition_kwargs=None, **rule):
        """recognize() with the words of every image grouped into text lines on the GPU (layout.group_lines with the
        detector's context; DESIGN.md section 4, "Lines").  Returns, per image, a list of ``(text, box, words)`` from the top
        of the page to its bottom: ``words`` are recognize()'s own ``(text, box)`` tuples of the line in reading order,
        ``text`` their texts joined by single spaces, ``box`` the (4, 2) float32 rectangle around the line along its axis.
        ``rule``: ``max_angle``, ``min_height_ratio``, ``max_offset``, ``max_gap`` as ``layout.group_lines``.
        ``beam_width`` / ``lexicon_top`` are refused (ValueError): their ``text`` is a list.  Columns are not detected:
        ``recognize_blocks`` reads a page column after column."""
        Extras.asked(recognition_kwargs).one_text_per_word("recognize_lines joins one text per word")
        predictions = self.recognize(images, detection_kwargs, recognition_kwargs)
        ctx = getattr(self.detector, "_ctx", None)
        pages = _layout.group_lines([[box for _, box in group] for group in predictions], ctx=ctx, **rule)
        return [[(" ".join(group[j][0] for j in line.words), line.box, [group[j] for j in line.words]) for line in lines]
                for group, lines in zip(predictions, pages)]

    def recognize_blocks(self, images, detection_kwargs=None, recognition_kwargs=None, min_gap_x=1.0, min_gap_y=0.75, **line_rule):
        """recognize_lines() with the lines of every image cut into blocks -- columns, paragraphs, headings -- in reading
        order on the GPU (layout.group_blocks on the line boxes, with the detector's context; DESIGN.md section 4,
        "Blocks"): two columns side by side are read one after the other.  Returns, per image, a list of ``(text, box,
        lines)`` in reading order: ``lines`` are recognize_lines()' own ``(text, box, words)`` tuples of the block from
        its top to its bottom, ``text`` their texts joined by ``"\\n"``, ``box`` the (4, 2) float32 axis-aligned box around
        them.  ``min_gap_x`` / ``min_gap_y`` as ``layout.group_blocks`` (judgement, not fitted to real pages);
        ``line_rule`` as ``recognize_lines``.  It refuses what recognize_lines() refuses.

        ``deskew=True`` (a keyword beside the line rule's, default False) is for rotated pages -- a skewed scan, a photo, a
        page fed in sideways or upside down: the page's text direction is estimated on the GPU from the line boxes
        handed to the cut, the cut runs in that frame (``layout.group_blocks_deskewed``; DESIGN.md section 4, "Rotated
        pages"), and ``box`` becomes a rotated rectangle whose tl -> tr runs along the text (``layout.box_angle``).  The
        rest of the return value keeps its shape."""
        deskew = line_rule.pop("deskew", False)
        if not isinstance(deskew, (bool, np.bool_)):
            raise TypeError(f"recognize_blocks: deskew must be True or False, not {deskew!r}")
        pages = self.recognize_lines(images, detection_kwargs, recognition_kwargs, **line_rule)
        ctx = getattr(self.detector, "_ctx", None)
        group = _layout.group_blocks_deskewed if deskew else _layout.group_blocks
        cut = group([[box for _, box, _ in lines] for lines in pages], ctx=ctx, min_gap_x=min_gap_x, min_gap_y=min_gap_y)
        return [[("\n".join(lines[j][0] for j in block.lines), block.box, [lines[j] for j in block.lines]) for block in blocks]
                for lines, blocks in zip(pages, cut)]

    def recognize_table(self, images, detection_kwargs=None, recognition_kwargs=None, **rule):
        """recognize() with the words of every image put into the rows, columns and spanning cells of a table on the GPU
        (layout.group_table with the detector's context; DESIGN.md section 4, "Tables").  Every image is ONE table: a
        price list, an invoice's item lines -- crop the table, or group the words of one block yourself.  Returns, per image,
        a ``layout.Table`` whose ``cells`` are in reading order; a cell's ``words`` are recognize()'s own ``(text, box)``
        tuples from left to right, its ``text`` their texts joined by single spaces; ``table.grid()`` is the rows x cols
        matrix of texts (``""`` where no word starts, a spanning cell's text at its first column).  ``rule``: ``min_gap_x``,
        ``min_gap_y``, ``min_support`` as ``layout.group_table`` (judgement, not fitted to real pages).  It refuses what
        recognize_blocks() refuses: ``beam_width`` / ``lexicon_top`` / ``pattern`` (ValueError), their ``text`` is no
        string."""
        Extras.asked(recognition_kwargs).one_text_per_word("recognize_table joins one text per word")
        unknown = set(rule) - {"min_gap_x", "min_gap_y", "min_support"}
        if unknown:
            raise TypeError(f"recognize_table: unknown rule parameter(s) {sorted(unknown)}")
        predictions = self.recognize(images, detection_kwargs, recognition_kwargs)
        ctx = getattr(self.detector, "_ctx", None)
        tables = _layout.group_table([[box for _, box in group] for group in predictions], ctx=ctx, **rule)
        return [table._replace(cells=[cell._replace(words=[group[j] for j in cell.words], text=" ".join(group[j][0] for j in cell.words))
                                      for cell in table.cells])
                for group, table in zip(predictions, tables)]

    def recognize_characters(self, images, detection_kwargs=None, recognition_kwargs=None, **rule):
        """recognize() with the character boxes of every word, read off the detector's region map on the GPU in the same
        pass ("Characters").  Returns, per image, a list of ``(text, box, characters)``: ``characters``
        is a ``layout.Characters(boxes (K, 4, 2) float32, scores (K,) float32)``, the characters from the box's tl towards
        its tr in input-image pixels (like ``box``, through ``tools.adjust_boxes``), and the region map's value at each
        character's peak.  Texts and word boxes are recognize()'s, bit for bit.  The detector counts blobs of its region
        map, the recogniser reads letters: ``characters.boxes[k]`` belongs to ``text[k]`` only when ``K == len(text)`` --
        the caller checks that.  ``rule``: ``peak_threshold``, ``valley_ratio``, ``extent_threshold`` as
        ``detection.get_char_boxes``.  ``beam_width`` / ``lexicon_top`` are refused (ValueError): their ``text`` is a list.
        A method of its own because recognize() keeps the reference's exact signature."""
        Extras.asked(recognition_kwargs).one_text_per_word("recognize_characters pairs one text per word with its characters")
        orientation_of(recognition_kwargs, char_boxes=True)  # ValueError naming both
        unknown = set(rule) - set(_lib.CHAR_RULE_DEFAULTS)
        if unknown:
            raise TypeError(f"recognize_characters: unknown rule parameter(s) {sorted(unknown)}")
        results = self._recognize(images, None, None, detection_kwargs, recognition_kwargs, char_boxes=_lib.char_rule(dict(rule)))
        return [[(text, box, characters) for (text, box), characters in zip(words, chars)]
                for words, chars in zip(self._assemble(results), results.characters)]

    def recognize_padded(self, images, hmax, wmax, detection_kwargs=None, recognition_kwargs=None, return_scores=False):
        """recognize() with the padded detector-input size imposed by the caller (used when a
        larger batch is sharded across GPUs: every shard pads to the WHOLE batch's size)."""
        return self._assemble(self._recognize(images, hmax, wmax, detection_kwargs, recognition_kwargs, return_scores))

    def recognize_raw(self, images, hmax=None, wmax=None, detection_kwargs=None, recognition_kwargs=None, return_scores=False,
                      char_boxes=None):
        """The fused device path up to (but not including) string assembly: ``Results.render_raw()`` -- ``(box_groups,
        label_rows)``, per image an (n_i,4,2) float32 array in INPUT-image pixels (adjust_boxes already applied,
        pipeline.py:66-71) and one (sum n_i, label width (48 by default)) int32 array of decoded label rows (-1 padded, recognition.py:177-182) in image
        order: the fixed-width form that crosses ranks in ``dist.ShardedPipeline``.  The extras follow as the fields of
        ``results.Results`` describe them: ``return_scores=True``, a ``beam_width`` or a ``lexicon_top`` in
        ``recognition_kwargs``, and ``char_boxes`` (True or a dict of rule parameters; ``layout.Characters`` in input-image
        pixels like the boxes)."""
        return self._recognize(images, hmax, wmax, detection_kwargs, recognition_kwargs, return_scores, char_boxes).render_raw()

    def _recognize(self, images, hmax, wmax, detection_kwargs, recognition_kwargs, return_scores=False, char_boxes=None):
        """recognize_raw's ``Results``, over one of three routes: the fused one, and the stage-wise one for images that are
        not uint8 or for foreign stages.  ``recognition_kwargs={"charset": name}``: every decode of the call runs under that
        character set of the recogniser (``Extras.charset_scope``); the boxes are the same either way."""
        extras = Extras.from_recognition_kwargs(self.recognizer, recognition_kwargs, return_scores, char_boxes)
        with extras.charset_scope(getattr(self.recognizer, "_ctx", None)):
            return self._recognize_routes(images, hmax, wmax, detection_kwargs, extras, (recognition_kwargs or {}).get("pattern"))

    def _recognize_routes(self, images, hmax, wmax, detection_kwargs, extras, pattern_name):
        if not isinstance(images, np.ndarray):
            images = [tools.read(image) for image in images]
        images = [np.ascontiguousarray(im) for im in images]
        if not images:
            return extras.empty_results(label_width_of(self.recognizer))
        detection_kwargs = dict(detection_kwargs or {})
        if extras.characters:
            detection_kwargs["char_boxes"] = extras.char_boxes
        ctx = getattr(self.detector, "_ctx", None)
        floats = any(im.dtype != np.uint8 for im in images)
        for feature in ("orientation", "pattern"):
            if getattr(extras, feature) is not None:
                only_uint8(images, feature)
        if floats or ctx is None or getattr(self.recognizer, "_ctx", None) is not ctx:
            # float (or any non-uint8) images: the reference's cv2 calls interpolate them in float (tools.py:394, :107); the
            # stage-wise path does the same with the float kernels (kocr_resize_pad_f32 / kocr_warp_crops_f32, round 5) -- off
            # the fused fixed-point path, which is defined for uint8 pixels only.  Duck-typed / separately-placed stages: the
            # reference's stage-wise path (pipeline.py:44-75)
            if extras.characters and "char_boxes" not in _scores.parameters(self.detector.detect):
                raise TypeError(f"char_boxes: the detector ({type(self.detector).__name__}.detect) cannot give character boxes "
                                "(it takes no char_boxes argument)")
            out, scales = self._recognize_stagewise([im.astype(np.float32) for im in images] if floats else images, detection_kwargs,
                                                    hmax, wmax, extras, pattern_name)
        else:
            scales, dhs, dws, hmax_, wmax_ = self._plan([im.shape for im in images])
            hmax = hmax_ if hmax is None else max(hmax, hmax_)
            wmax = wmax_ if wmax is None else max(wmax, wmax_)
            out = self._fused(ctx.pipeline, images, dhs, dws, (hmax, wmax), detection_kwargs, extras)
        return self._to_input_pixels(out, scales, extras)

    @staticmethod
    def _fused(call, images, dhs, dws, sizes, detection_kwargs, extras):
        """One fused call (``Context.pipeline`` with ``sizes`` = (hmax, wmax), ``Context.pipeline_tiled`` with (tile, overlap))
        on uint8 images -> its ``Results``, boxes and characters in detector-input pixels"""
        micro_batch = detection_kwargs.pop("batch_size", 0) or 0
        out = Results.parse_context(call(
            images, [im.shape[0] for im in images], [im.shape[1] for im in images], dhs, dws, *sizes,
            micro_batch=micro_batch, return_scores=extras.scores, beam=extras.beam, lexicon_top=extras.lexicon_top,
            **({} if extras.orientation is None else {"orientation": extras.orientation}),
            **({} if extras.pattern is None else {"pattern": extras.pattern}), **detection_kwargs), *extras.flags())
        if extras.characters:
            out.characters = _layout.characters_of(out.characters)
        return out

    def _to_input_pixels(self, out, scales, extras):
        """``Results`` in detector-input pixels -> the same in input-image pixels (pipeline.py:66-71), an oriented run's boxes
        replaced by its quads"""
        if extras.orientation is not None:
            # every word's box becomes its oriented quad: the same corners, renamed
            turns, quads, log_words = out.orientation
            ends = np.cumsum([len(b) for b in out.boxes])
            out.boxes = [quads[end - len(b):end] if len(b) else b for b, end in zip(out.boxes, ends)]
        out.boxes = self._adjust(out.boxes, scales)
        if extras.orientation is not None:
            filled = [b for b in out.boxes if len(b)]
            out.orientation = (turns, np.concatenate(filled) if filled else quads, log_words)
        if extras.characters:
            out.characters = [[_layout.Characters(self._adjust([c.boxes], [scale])[0], c.scores) for c in page]
                              for page, scale in zip(out.characters, scales)]
        return out

    def recognize_tiled(self, images, tile=1024, overlap=128, scale=None, detection_kwargs=None, recognition_kwargs=None,
                        return_scores=False, char_boxes=None):
        """recognize() for pages larger than the detector takes in one image, such as a scanned document at its own
        resolution ("Tiled pages").  Every page is resized by ``scale`` (default ``self.scale``) to
        ``int(h * scale) x int(w * scale)`` -- ``max_size`` does not apply -- and read in a call of its own: the detector runs
        on overlapping ``tile`` x ``tile`` pieces of the page, ``overlap`` pixels of halo on every inner side
        (``tools.tile_plan``), ``detection_kwargs["batch_size"]`` tiles at a time; their heat-maps are stitched in HBM and
        everything behind them is recognize()'s own path.  Returns what recognize() returns, boxes in input-image pixels; with
        ``return_scores`` the tuples are ``recognize_with_scores``', with ``char_boxes`` (True or a dict of rule parameters)
        ``recognize_characters``' (not both).  ``recognition_kwargs`` takes ``beam_width`` / ``top_paths``, ``lexicon_top`` and
        ``orientation`` / ``tall_ratio`` and ``charset`` as recognize() does, with the same refusals.  uint8 images only
        (NotImplementedError); detector and recogniser must share one ``Context`` (TypeError).  A halo narrower than the
        detector's receptive field does not reproduce a whole-page pass exactly: see DESIGN.md."""
        extras = Extras.from_recognition_kwargs(self.recognizer, recognition_kwargs, return_scores, char_boxes, tiled=True)
        with extras.charset_scope(getattr(self.recognizer, "_ctx", None)):
            return self._recognize_tiled(images, tile, overlap, scale, detection_kwargs, extras)

    def _recognize_tiled(self, images, tile, overlap, scale, detection_kwargs, extras):
        if not isinstance(images, np.ndarray):
            images = [tools.read(image) for image in images]
        images = [np.ascontiguousarray(im) for im in images]
        ctx = getattr(self.detector, "_ctx", None)
        if ctx is None or not hasattr(ctx, "pipeline_tiled"):
            raise TypeError(f"recognize_tiled: the detector ({type(self.detector).__name__}) has no libkocr context to run tiles on")
        if getattr(self.recognizer, "_ctx", None) is not ctx:
            raise TypeError(f"recognize_tiled: the recognizer ({type(self.recognizer).__name__}) is not on the detector's context")
        only_uint8(images, "recognize_tiled")
        tools.tile_plan(1, 1, tile, overlap)  # ValueError for a refused tile or overlap, pages or not
        scale = self.scale if scale is None else scale
        pages = []
        for im in images:
            kwargs = dict(detection_kwargs or {})
            if extras.characters:
                kwargs["char_boxes"] = extras.char_boxes
            out = self._fused(ctx.pipeline_tiled, [im], [int(im.shape[0] * scale)], [int(im.shape[1] * scale)], (tile, overlap), kwargs,
                              extras)
            out = self._to_input_pixels(out, [scale], extras)
            words = self._assemble(out)[0]
            pages.append([(text, box, characters) for (text, box), characters in zip(words, out.characters[0])] if extras.characters
                         else words)
        return pages

    def _recognize_stagewise(self, images, detection_kwargs, hmax, wmax, extras, pattern=None):
        """pipeline.py:44-75 with the public stage APIs only (any object with ``detect`` /
        ``recognize_from_boxes``); strings are mapped back to label rows through the recognizer's alphabet.
        ``hmax`` / ``wmax``: padded size imposed by the caller (a sharded batch pads to the WHOLE batch's size).
        With ``char_boxes`` in ``detection_kwargs``, ``detect`` also returns its character groups.  Returns the ``Results``,
        boxes and characters still in detector-input pixels, and the scale of every page.
        The label rows, and the character-score, beam and pattern rows beside them, have the recogniser's label width
        (``label_width_of``), as the fused route's; a text longer than that is a ValueError.  A duck-typed recogniser that
        reports no width keeps ``max(48, longest text)`` columns.  ``pattern``: the name ``extras.pattern`` was resolved from."""
        return_scores, beam, lexicon_top, orientation = extras.scores, extras.beam, extras.lexicon_top, extras.orientation
        own = getattr(self.detector, "_ctx", None)  # a libkocr-backed detector: its context also resizes (else the default one)
        resized = [tools.resize_image(image, max_scale=self.scale, max_size=self.max_size, **({"ctx": own} if own is not None else {}))
                   for image in images]
        max_height, max_width = np.array([image.shape[:2] for image, _ in resized]).max(axis=0)
        max_height = max(int(max_height), int(hmax or 0))
        max_width = max(int(max_width), int(wmax or 0))
        padded = np.array([tools.pad(image, width=max_width, height=max_height) for image, _ in resized])
        with_characters = extras.characters
        turned = {}
        if orientation is not None:
            # passed on only to a recogniser that takes the two arguments
            takes = _scores.parameters(self.recognizer.recognize_from_boxes)
            if "orientation" not in takes or "tall_ratio" not in takes or "return_orientation" not in takes:
                raise TypeError(f"orientation: the recognizer ({type(self.recognizer).__name__}.recognize_from_boxes) cannot read "
                                "boxes in two orientations (it takes no orientation / tall_ratio / return_orientation argument)")
            turned = {"orientation": orientation[0], "tall_ratio": orientation[1], "return_orientation": True}
        how = []
        if return_scores:
            detect = _scores.need("detector", self.detector, "detect")
            recognize = _scores.need("recognizer", self.recognizer, "recognize_from_boxes")
            detected = detect(images=padded, return_scores=True, **detection_kwargs)
            pairs = [pair for group in recognize(images=padded, box_groups=detected[0], return_scores=True, **turned) for pair in group]
            if turned:
                how = [o for _, _, o in pairs]
                pairs = [(t, score) for t, score, _ in pairs]
            rows = [t for t, _ in pairs]
        else:
            detected = self.detector.detect(images=padded, **detection_kwargs)
            detected = detected if with_characters else (detected,)
            rows = [t for group in self.recognizer.recognize_from_boxes(images=padded, box_groups=detected[0], **turned) for t in group]
            if turned:
                how = [o for _, o in rows]
                rows = [t for t, _ in rows]
        alphabet = self.recognizer.alphabet
        width = label_width_of(self.recognizer)
        if width is None:
            width = max([48] + [len(t) for t in rows])
        elif any(len(t) > width for t in rows):
            raise ValueError(f"the recognizer reports a label width of {width} but returned a text of {max(len(t) for t in rows)} characters")
        out = Results(detected[0], np.full((len(rows), width), -1, np.int32),
                      characters=detected[-1] if with_characters else None)
        for r, t in enumerate(rows):
            out.labels[r, :len(t)] = [alphabet.index(ch) for ch in t]
        if beam:
            # a second recogniser call: the public method returns either the decode or its alternatives
            words = [w for group in self.recognizer.recognize_from_boxes(images=padded, box_groups=out.boxes, beam_width=beam[0],
                                                                         top_paths=beam[1]) for w in group]
            out.beam = (np.full((len(rows), beam[1], out.labels.shape[1]), -1, np.int32),
                        np.full((len(rows), beam[1]), -np.inf, np.float32))
            for r, alternatives in enumerate(words):
                for k, (t, log_prob) in enumerate(alternatives):
                    out.beam[0][r, k, :len(t)] = [alphabet.index(ch) for ch in t]
                    out.beam[1][r, k] = log_prob
        if lexicon_top:
            # likewise a second recogniser call; the words go back to their indices in the recogniser's lexicon
            where = {word: v for v, word in enumerate(self.recognizer.lexicon.words)}
            out.lexicon = (np.full((len(rows), lexicon_top), -1, np.int32), np.full((len(rows), lexicon_top), -np.inf, np.float32))
            matched = self.recognizer.recognize_from_boxes(images=padded, box_groups=out.boxes, lexicon_top=lexicon_top)
            for r, matches in enumerate(m for group in matched for m in group):
                for k, (word, log_prob) in enumerate(matches):
                    out.lexicon[0][r, k] = where[word]
                    out.lexicon[1][r, k] = log_prob
        if pattern is not None:
            # likewise a second recogniser call (``pattern``: the name); the public method gives no log_path: NaN
            read = [w for group in self.recognizer.recognize_from_boxes(images=padded, box_groups=out.boxes, pattern=pattern) for w in group]
            out.pattern = (np.full(out.labels.shape, -1, np.int32), np.full(len(rows), np.nan, np.float32),
                           np.full(len(rows), -np.inf, np.float32))
            for r, (t, log_prob) in enumerate(read):
                if t is not None:
                    out.pattern[0][r, :len(t)] = [alphabet.index(ch) for ch in t]
                    out.pattern[2][r] = log_prob
        if return_scores:
            chars = np.zeros(out.labels.shape, np.float32)
            for r, (_, score) in enumerate(pairs):
                chars[r, :len(score.characters)] = score.characters
            out.scores = ([np.asarray(d, np.float32) for d in detected[1]], np.array([score.log_word for _, score in pairs], np.float32), chars)
        if turned:
            out.orientation = (np.array([o.turns for o in how], np.int32), np.array([o.box for o in how], np.float32).reshape(-1, 4, 2),
                               np.array([o.log_words for o in how], np.float32).reshape(-1, 2))
        return out, [scale for _, scale in resized]

    def recognize_windowed(self, images, aspect=10.0, overlap=40, detection_kwargs=None, return_scores=False):
        """recognize() with long words read in overlapping windows ("Long words"): the detector runs as
        in recognize(), then ``Recognizer.recognize_from_boxes_windowed`` reads its boxes -- a box wider than ``aspect`` times
        its height in windows stitched on the GPU, every other box as ever.  The stage-wise route (resize, detect, windowed
        recogniser), not the fused call.  Returns what recognize() returns, (text, box) tuples per image with the boxes in
        input-image pixels -- recognize()'s boxes, and its texts for every box that is not long --, or, with
        ``return_scores=True``, recognize_with_scores()' (text, box, score) tuples.  uint8 images only (NotImplementedError)."""
        read = getattr(self.recognizer, "recognize_from_boxes_windowed", None)
        if read is None:
            raise TypeError(f"the recognizer ({type(self.recognizer).__name__}) cannot read boxes in windows (it has no "
                            "recognize_from_boxes_windowed method)")
        if not isinstance(images, np.ndarray):
            images = [tools.read(image) for image in images]
        images = [np.ascontiguousarray(im) for im in images]
        only_uint8(images, "windowed")
        if not images:
            return []
        own = getattr(self.detector, "_ctx", None)
        resized = [tools.resize_image(image, max_scale=self.scale, max_size=self.max_size, **({"ctx": own} if own is not None else {}))
                   for image in images]
        max_height, max_width = np.array([image.shape[:2] for image, _ in resized]).max(axis=0)
        padded = np.array([tools.pad(image, width=int(max_width), height=int(max_height)) for image, _ in resized])
        detection_kwargs = dict(detection_kwargs or {})
        if return_scores:
            box_groups, detection = _scores.need("detector", self.detector, "detect")(images=padded, return_scores=True, **detection_kwargs)
        else:
            box_groups, detection = self.detector.detect(images=padded, **detection_kwargs), None
        words = read(padded, box_groups, aspect=aspect, overlap=overlap, return_scores=return_scores)
        adjusted = self._adjust(box_groups, [scale for _, scale in resized])
        if not return_scores:
            return [list(zip(texts, boxes)) for texts, boxes in zip(words, adjusted)]
        return [[(text, box, score._replace(detection=float(d))) for (text, score), box, d in zip(group, boxes, np.asarray(det).reshape(-1))]
                for group, boxes, det in zip(words, adjusted, detection)]

    def recognize_device(self, d_ptr, n, h, w, detection_kwargs=None, return_scores=False):
        """Same as recognize() for a batch already resident in HBM: ``d_ptr`` = device pointer of an
        (n,h,w,3) uint8 tensor (e.g. ``torch.Tensor.data_ptr()``)."""
        return self._assemble(self._recognize_device(d_ptr, n, h, w, detection_kwargs, None, return_scores))

    def recognize_device_raw(self, d_ptr, n, h, w, detection_kwargs=None, device_results=None, return_scores=False):
        """recognize_device up to (but not including) string assembly: ``(box_groups, label_rows[, scores])`` as recognize_raw.
        ``device_results`` (a dict, optional) receives where the same results still lie in HBM (``Context.
        pipeline_device_results``: boxes in DETECTOR-input pixels, before the division by the scale) plus ``scale``, for a
        caller that packs them on the device (``dist.gather_packed``); valid until the next call on the context."""
        return self._recognize_device(d_ptr, n, h, w, detection_kwargs, device_results, return_scores).render_raw()

    def _recognize_device(self, d_ptr, n, h, w, detection_kwargs, device_results, return_scores):
        detection_kwargs = dict(detection_kwargs or {})
        ctx = self.detector._ctx  # pylint: disable=protected-access
        scales, dhs, dws, hmax, wmax = self._plan([(h, w, 3)] * n)
        micro_batch = detection_kwargs.pop("batch_size", 0) or 0
        stride = h * w * 3
        out = Results.parse_context(ctx.pipeline([int(d_ptr) + i * stride for i in range(n)], [h] * n, [w] * n, dhs, dws,
                                                 hmax, wmax, micro_batch=micro_batch, on_device=True, return_scores=return_scores,
                                                 **detection_kwargs), return_scores)
        if device_results is not None and n:
            device_results.update(ctx.pipeline_device_results())
            device_results["scale"] = scales[0]  # one size, one scale
        out.boxes = self._adjust(out.boxes, scales)
        return out

    @staticmethod
    def _adjust(box_groups, scales):
        """pipeline.py:66-71: boxes back to input-image pixels (identity when scale == 1)."""
        return [
            tools.adjust_boxes(boxes=boxes, boxes_format="boxes", scale=1 / scale) if scale != 1 else boxes
            for boxes, scale in zip(box_groups, scales)
        ]

    def assemble(self, box_groups, labels, score_rows=None, beam_rows=None, lexicon_rows=None):
        """(box_groups, label rows) -> the reference's return value (pipeline.py:72-75); the other arguments are
        recognize_raw's third to fifth elements, the ``scores``, ``beam`` and ``lexicon`` of ``results.Results``: with
        ``score_rows`` every tuple gets its ``scores.Score``; with ``beam_rows`` the texts are replaced by their lists of
        ``(text, log_prob)`` alternatives; with ``lexicon_rows`` by their lists of ``(word, log_prob)`` matches, the words looked
        up in ``recognizer.lexicon.words``."""
        return self._assemble(Results(box_groups, labels, score_rows, beam_rows, lexicon_rows))

    def _assemble(self, results):
        # recognition.py:527-534: label rows -> strings, skipping the blank (= len(alphabet)) and the -1 padding
        predictions, scores = results.words(self.recognizer.alphabet, getattr(self.recognizer, "lexicon", None))
        columns = [] if scores is None else [scores]
        out, start = [], 0
        for boxes in results.boxes:
            out.append(list(zip(predictions[start:start + len(boxes)], boxes, *[c[start:start + len(boxes)] for c in columns])))
            start += len(boxes)
        return out
