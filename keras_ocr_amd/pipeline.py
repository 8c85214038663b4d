"""Host-side mirror of ``keras_ocr.pipeline.Pipeline`` (reference ``keras_ocr/pipeline.py:7-75``)."""
import numpy as np

from . import _lib, detection, evaluation as _evaluation, layout as _layout, lexicon as _lexicon, recognition, scores as _scores, tools


def beam_of(recognition_kwargs):
    """``(beam_width, top_paths)`` from recognize()'s ``recognition_kwargs`` (validated: ValueError naming the argument), or
    None without a ``beam_width``.  Every other key is a Keras predict argument and has no effect on results."""
    kwargs = recognition_kwargs or {}
    if kwargs.get("beam_width") is None:
        return None
    return _lib.beam_args(kwargs["beam_width"], kwargs.get("top_paths", 1))


def lexicon_of(recognition_kwargs):
    """``lexicon_top`` from recognize()'s ``recognition_kwargs`` (validated: ValueError naming the argument, or saying that
    it cannot be combined with ``beam_width``), or None without one."""
    kwargs = recognition_kwargs or {}
    if kwargs.get("lexicon_top") is None:
        return None
    if kwargs.get("beam_width") is not None:
        raise ValueError("lexicon_top and beam_width cannot be combined: ask for one of the two")
    return _lexicon.top_arg(kwargs["lexicon_top"])


def decode_labels(alphabet, labels):
    """Label rows -> strings, skipping the blank (= len(alphabet)) and the -1 padding (recognition.py:527-534).

    One table lookup and one UTF-32 decode for the whole batch: iterating 600 x 48 numpy scalars costs 4 ms
    per call, during which the GPU sits idle."""
    labels = np.asarray(labels)
    if labels.size == 0:
        return [""] * len(labels)
    n = len(alphabet)
    if (labels.ndim != 2 or any(len(c) != 1 or c == "\0" or 0xD800 <= ord(c) <= 0xDFFF for c in alphabet)
            or labels.min() < -1 or labels.max() > n):
        # multi-character entries, lone surrogates (no UTF-32 encoding), a single row, or indices the reference's own
        # expression would wrap / reject: evaluate that expression
        skip = (n, -1)
        rows = labels.tolist() if labels.ndim == 2 else [labels.tolist()] if labels.ndim == 1 else labels.reshape(-1, labels.shape[-1]).tolist()
        return ["".join([alphabet[i] for i in row if i not in skip]) for row in rows]
    table = np.array([ord(c) for c in alphabet] + [0], "<u4")
    text = table[np.where(labels < 0, n, labels)].tobytes().decode("utf-32-le")
    w = labels.shape[1]
    return [text[i * w:(i + 1) * w].replace("\0", "") for i in range(labels.shape[0])]


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
        keys of both dicts are Keras predict arguments without effect."""
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
        for key in ("beam_width", "lexicon_top"):
            if (recognition_kwargs or {}).get(key) is not None:
                raise ValueError(f"evaluate scores one text per word: {key} in recognition_kwargs makes every text a list of alternatives")
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
        ``beam_width`` / ``lexicon_top`` are refused (ValueError): their ``text`` is a list."""
        for key in ("beam_width", "lexicon_top"):
            if (recognition_kwargs or {}).get(key) is not None:
                raise ValueError(f"recognize_lines joins one text per word: {key} in recognition_kwargs makes every text a list of alternatives")
        predictions = self.recognize(images, detection_kwargs, recognition_kwargs)
        ctx = getattr(self.detector, "_ctx", None)
        pages = _layout.group_lines([[box for _, box in group] for group in predictions], ctx=ctx, **rule)
        return [[(" ".join(group[j][0] for j in line.words), line.box, [group[j] for j in line.words]) for line in lines]
                for group, lines in zip(predictions, pages)]

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
        for key in ("beam_width", "lexicon_top"):
            if (recognition_kwargs or {}).get(key) is not None:
                raise ValueError(f"recognize_characters pairs one text per word with its characters: {key} in recognition_kwargs makes "
                                 "every text a list of alternatives")
        unknown = set(rule) - set(_lib.CHAR_RULE_DEFAULTS)
        if unknown:
            raise TypeError(f"recognize_characters: unknown rule parameter(s) {sorted(unknown)}")
        box_groups, labels, char_groups = self.recognize_raw(images, None, None, detection_kwargs, recognition_kwargs,
                                                             char_boxes=_lib.char_rule(dict(rule)))
        return [[(text, box, characters) for (text, box), characters in zip(words, chars)]
                for words, chars in zip(self.assemble(box_groups, labels), char_groups)]

    def recognize_padded(self, images, hmax, wmax, detection_kwargs=None, recognition_kwargs=None, return_scores=False):
        """recognize() with the padded detector-input size imposed by the caller (used when a
        larger batch is sharded across GPUs: every shard pads to the WHOLE batch's size)."""
        return self.assemble(*self.recognize_raw(images, hmax, wmax, detection_kwargs, recognition_kwargs, return_scores))

    def recognize_raw(self, images, hmax=None, wmax=None, detection_kwargs=None, recognition_kwargs=None, return_scores=False,
                      char_boxes=None):
        """The fused device path up to (but not including) string assembly: returns
        ``(box_groups, label_rows)`` -- per image an (n_i,4,2) float32 array in INPUT-image pixels
        (adjust_boxes already applied, pipeline.py:66-71) and one (sum n_i, 48) int32 array of decoded
        label rows (-1 padded, recognition.py:177-182) in image order.  This fixed-width form is what
        crosses ranks in ``dist.ShardedPipeline``.  ``return_scores=True`` adds a third element ``(detection, log_word,
        char_scores)``: per image an (n_i,) float32 array, and (sum n_i,) / (sum n_i, 48) float32 arrays in label-row order.
        With a ``beam_width`` in ``recognition_kwargs`` the result has four elements: the third is the scores or None, the
        fourth ``(beam labels (sum n_i, K, 48) int32, beam log_prob (sum n_i, K) float32)`` as ``Context.crnn_beam``.  With a
        ``lexicon_top`` it has five: scores or None, None, ``(index (sum n_i, K) int32, log_prob (sum n_i, K) float32)`` as
        ``Context.crnn_lexicon``.  ``char_boxes`` (True or a dict of rule parameters): a very last element, per image one
        ``layout.Characters`` per box, in input-image pixels like the boxes."""
        if char_boxes is not None and char_boxes is not False:
            return self._recognize_raw_characters(images, hmax, wmax, detection_kwargs, recognition_kwargs, return_scores, char_boxes)
        if not isinstance(images, np.ndarray):
            images = [tools.read(image) for image in images]
        images = [np.ascontiguousarray(im) for im in images]
        lexicon_top = lexicon_of(recognition_kwargs)
        beam = beam_of(recognition_kwargs)  # the rest: Keras predict kwargs, no effect on results
        if lexicon_top is not None and getattr(self.recognizer, "lexicon", None) is None:
            raise ValueError("lexicon_top needs a loaded lexicon: call recognizer.set_lexicon(words) first")
        if not images:
            empty = [], np.zeros((0, 48), np.int32)
            scores = ([], np.zeros(0, np.float32), np.zeros((0, 48), np.float32)) if return_scores else None
            if lexicon_top:
                return empty + (scores, None, (np.zeros((0, lexicon_top), np.int32), np.zeros((0, lexicon_top), np.float32)))
            if beam:
                return empty + (scores, (np.zeros((0, beam[1], 48), np.int32), np.zeros((0, beam[1]), np.float32)))
            return empty + (scores,) if return_scores else empty
        detection_kwargs = dict(detection_kwargs or {})
        ctx = getattr(self.detector, "_ctx", None)
        if any(im.dtype != np.uint8 for im in images):
            # float (or any non-uint8) images: the reference's cv2 calls interpolate them in float (tools.py:394, :107);
            # the stage-wise path does the same with the float kernels (kocr_resize_pad_f32 / kocr_warp_crops_f32, round 5) --
            # off the fused fixed-point path, which is defined for uint8 pixels only
            return self._recognize_stagewise([im.astype(np.float32) for im in images], detection_kwargs, hmax, wmax, return_scores,
                                             beam, lexicon_top)
        if ctx is None or getattr(self.recognizer, "_ctx", None) is not ctx:
            # duck-typed / separately-placed stages: the reference's stage-wise path (pipeline.py:44-75)
            return self._recognize_stagewise(images, detection_kwargs, hmax, wmax, return_scores, beam, lexicon_top)
        scales, dhs, dws, hmax_, wmax_ = self._plan([im.shape for im in images])
        hmax = hmax_ if hmax is None else max(hmax, hmax_)
        wmax = wmax_ if wmax is None else max(wmax, wmax_)
        micro_batch = detection_kwargs.pop("batch_size", 0) or 0
        box_groups, *rest = ctx.pipeline(
            images, [im.shape[0] for im in images], [im.shape[1] for im in images], dhs, dws, hmax, wmax,
            micro_batch=micro_batch, return_scores=return_scores, beam=beam, lexicon_top=lexicon_top, **detection_kwargs)
        if (beam or lexicon_top) and not return_scores:
            rest.insert(1, None)
        if lexicon_top:
            rest.insert(2, None)
        return (self._adjust(box_groups, scales), *rest)

    def _recognize_raw_characters(self, images, hmax, wmax, detection_kwargs, recognition_kwargs, return_scores, char_boxes):
        """recognize_raw with ``char_boxes``: the same routes, the detector also asked for its character boxes"""
        if not isinstance(images, np.ndarray):
            images = [tools.read(image) for image in images]
        images = [np.ascontiguousarray(im) for im in images]
        if not images:
            return self.recognize_raw(images, hmax, wmax, detection_kwargs, recognition_kwargs, return_scores) + ([],)
        detection_kwargs = dict(detection_kwargs or {})
        ctx = getattr(self.detector, "_ctx", None)
        stagewise = any(im.dtype != np.uint8 for im in images) or ctx is None or getattr(self.recognizer, "_ctx", None) is not ctx
        if stagewise:
            import inspect

            try:
                params = inspect.signature(self.detector.detect).parameters
            except (TypeError, ValueError):
                params = {}
            if "char_boxes" not in params:
                raise TypeError(f"char_boxes: the detector ({type(self.detector).__name__}.detect) cannot give character boxes "
                                "(it takes no char_boxes argument)")
            detection_kwargs["char_boxes"] = char_boxes
            # the stage-wise route calls detector.detect(**detection_kwargs): its result then ends with the character groups
            *head, scales, char_groups = self._recognize_stagewise(
                [im.astype(np.float32) for im in images] if any(im.dtype != np.uint8 for im in images) else images,
                detection_kwargs, hmax, wmax, return_scores,
                beam_of(recognition_kwargs), lexicon_of(recognition_kwargs), with_characters=True)
        else:
            scales, dhs, dws, hmax_, wmax_ = self._plan([im.shape for im in images])
            hmax = hmax_ if hmax is None else max(hmax, hmax_)
            wmax = wmax_ if wmax is None else max(wmax, wmax_)
            micro_batch = detection_kwargs.pop("batch_size", 0) or 0
            lexicon_top, beam = lexicon_of(recognition_kwargs), beam_of(recognition_kwargs)
            box_groups, *rest, groups = ctx.pipeline(
                images, [im.shape[0] for im in images], [im.shape[1] for im in images], dhs, dws, hmax, wmax,
                micro_batch=micro_batch, return_scores=return_scores, beam=beam, lexicon_top=lexicon_top, char_boxes=char_boxes,
                **detection_kwargs)
            if (beam or lexicon_top) and not return_scores:
                rest.insert(1, None)
            if lexicon_top:
                rest.insert(2, None)
            head = [self._adjust(box_groups, scales), *rest]
            char_groups = _layout.characters_of(groups)
        adjusted = [[_layout.Characters(tools.adjust_boxes(boxes=c.boxes, boxes_format="boxes", scale=1 / scale) if scale != 1 else c.boxes,
                                        c.scores) for c in page] for page, scale in zip(char_groups, scales)]
        return (*head, adjusted)

    def _recognize_stagewise(self, images, detection_kwargs, hmax=None, wmax=None, return_scores=False, beam=None, lexicon_top=None,
                             with_characters=False):
        """pipeline.py:44-75 with the public stage APIs only (any object with ``detect`` /
        ``recognize_from_boxes``); strings are mapped back to label rows through the recognizer's alphabet.
        ``hmax`` / ``wmax``: padded size imposed by the caller (a sharded batch pads to the WHOLE batch's size).
        ``with_characters``: ``detection_kwargs`` holds ``char_boxes``, so ``detect`` also returns its character groups; the
        result then ends with ``scales, char_groups`` (the groups still in detector-input pixels)."""
        own = getattr(self.detector, "_ctx", None)  # a libkocr-backed detector: its context also resizes (else the default one)
        resized = [tools.resize_image(image, max_scale=self.scale, max_size=self.max_size, **({"ctx": own} if own is not None else {}))
                   for image in images]
        max_height, max_width = np.array([image.shape[:2] for image, _ in resized]).max(axis=0)
        max_height = max(int(max_height), int(hmax or 0))
        max_width = max(int(max_width), int(wmax or 0))
        scales = [scale for _, scale in resized]
        padded = np.array([tools.pad(image, width=max_width, height=max_height) for image, _ in resized])
        if return_scores:
            detect = _scores.need("detector", self.detector, "detect")
            recognize = _scores.need("recognizer", self.recognizer, "recognize_from_boxes")
            box_groups, det, *char_groups = detect(images=padded, return_scores=True, **detection_kwargs)
            pairs = [pair for group in recognize(images=padded, box_groups=box_groups, return_scores=True) for pair in group]
            rows = [t for t, _ in pairs]
        else:
            box_groups = self.detector.detect(images=padded, **detection_kwargs)
            if with_characters:
                box_groups, *char_groups = box_groups
            texts = self.recognizer.recognize_from_boxes(images=padded, box_groups=box_groups)
            rows = [t for group in texts for t in group]
        alphabet = self.recognizer.alphabet
        labels = np.full((len(rows), max([48] + [len(t) for t in rows])), -1, np.int32)
        for r, t in enumerate(rows):
            labels[r, :len(t)] = [alphabet.index(ch) for ch in t]
        if beam:
            # a second recogniser call: the public method returns either the decode or its alternatives
            words = [w for group in self.recognizer.recognize_from_boxes(images=padded, box_groups=box_groups, beam_width=beam[0],
                                                                         top_paths=beam[1]) for w in group]
            beam_rows = (np.full((len(rows), beam[1], labels.shape[1]), -1, np.int32),
                         np.full((len(rows), beam[1]), -np.inf, np.float32))
            for r, alternatives in enumerate(words):
                for k, (t, log_prob) in enumerate(alternatives):
                    beam_rows[0][r, k, :len(t)] = [alphabet.index(ch) for ch in t]
                    beam_rows[1][r, k] = log_prob
        if lexicon_top:
            # likewise a second recogniser call; the words go back to their indices in the recogniser's lexicon
            where = {word: v for v, word in enumerate(self.recognizer.lexicon.words)}
            lexicon_rows = (np.full((len(rows), lexicon_top), -1, np.int32), np.full((len(rows), lexicon_top), -np.inf, np.float32))
            matched = self.recognizer.recognize_from_boxes(images=padded, box_groups=box_groups, lexicon_top=lexicon_top)
            for r, matches in enumerate(m for group in matched for m in group):
                for k, (word, log_prob) in enumerate(matches):
                    lexicon_rows[0][r, k] = where[word]
                    lexicon_rows[1][r, k] = log_prob
        if return_scores:
            chars = np.zeros(labels.shape, np.float32)
            for r, (_, score) in enumerate(pairs):
                chars[r, :len(score.characters)] = score.characters
            log_word = np.array([score.log_word for _, score in pairs], np.float32)
            score_rows = ([np.asarray(d, np.float32) for d in det], log_word, chars)
            out = (self._adjust(box_groups, scales), labels, score_rows) + ((beam_rows,) if beam else ()) + \
                ((None, lexicon_rows) if lexicon_top else ())
        else:
            out = (self._adjust(box_groups, scales), labels) + ((None, beam_rows) if beam else ()) + \
                ((None, None, lexicon_rows) if lexicon_top else ())
        return out + (scales, char_groups[0]) if with_characters else out

    def recognize_device(self, d_ptr, n, h, w, detection_kwargs=None, return_scores=False):
        """Same as recognize() for a batch already resident in HBM: ``d_ptr`` = device pointer of an
        (n,h,w,3) uint8 tensor (e.g. ``torch.Tensor.data_ptr()``)."""
        return self.assemble(*self.recognize_device_raw(d_ptr, n, h, w, detection_kwargs, return_scores=return_scores))

    def recognize_device_raw(self, d_ptr, n, h, w, detection_kwargs=None, device_results=None, return_scores=False):
        """recognize_device up to (but not including) string assembly: ``(box_groups, label_rows)`` as recognize_raw.
        ``device_results`` (a dict, optional) receives where the same results still lie in HBM (``Context.
        pipeline_device_results``: boxes in DETECTOR-input pixels, before the division by the scale) plus ``scale``, for a
        caller that packs them on the device (``dist.gather_packed``); valid until the next call on the context."""
        detection_kwargs = dict(detection_kwargs or {})
        ctx = self.detector._ctx  # pylint: disable=protected-access
        scales, dhs, dws, hmax, wmax = self._plan([(h, w, 3)] * n)
        micro_batch = detection_kwargs.pop("batch_size", 0) or 0
        stride = h * w * 3
        box_groups, *rest = ctx.pipeline([int(d_ptr) + i * stride for i in range(n)], [h] * n, [w] * n, dhs, dws,
                                         hmax, wmax, micro_batch=micro_batch, on_device=True, return_scores=return_scores,
                                         **detection_kwargs)
        if device_results is not None and n:
            device_results.update(ctx.pipeline_device_results())
            device_results["scale"] = scales[0]  # one size, one scale
        return (self._adjust(box_groups, scales), *rest)

    @staticmethod
    def _adjust(box_groups, scales):
        """pipeline.py:66-71: boxes back to input-image pixels (identity when scale == 1)."""
        return [
            tools.adjust_boxes(boxes=boxes, boxes_format="boxes", scale=1 / scale) if scale != 1 else boxes
            for boxes, scale in zip(box_groups, scales)
        ]

    def assemble(self, box_groups, labels, score_rows=None, beam_rows=None, lexicon_rows=None):
        """(box_groups, label rows) -> the reference's return value (pipeline.py:72-75); with ``score_rows`` (recognize_raw's
        third element) every tuple gets its ``scores.Score``; with ``beam_rows`` (its fourth) the texts are replaced by
        their lists of ``(text, log_prob)`` alternatives; with ``lexicon_rows`` (its fifth) by their lists of ``(word,
        log_prob)`` matches, the words looked up in ``recognizer.lexicon.words``."""
        # recognition.py:527-534: label rows -> strings, skipping the blank (= len(alphabet)) and the -1 padding
        if lexicon_rows is not None:
            words = self.recognizer.lexicon.words
            predictions = [[(words[i], float(v)) for i, v in zip(row, vals) if i >= 0]
                           for row, vals in zip(np.asarray(lexicon_rows[0]).tolist(), np.asarray(lexicon_rows[1]))]
        elif beam_rows is not None:
            beam_labels, beam_log_prob = np.asarray(beam_rows[0]), np.asarray(beam_rows[1])
            m, k = beam_log_prob.shape
            texts = decode_labels(self.recognizer.alphabet, beam_labels.reshape(m * k, -1)) if m * k else []
            predictions = [[(texts[i * k + j], float(beam_log_prob[i, j])) for j in range(k) if beam_log_prob[i, j] != -np.inf]
                           for i in range(m)]
        else:
            predictions = decode_labels(self.recognizer.alphabet, labels)
        columns = [predictions]
        if score_rows is not None:
            det, log_word, chars = score_rows
            flat = np.concatenate([np.asarray(d, np.float32).reshape(-1) for d in det]) if len(det) else np.zeros(0, np.float32)
            columns.append(_scores.assemble(labels, log_word, chars, flat))
        out, start = [], 0
        for boxes in box_groups:
            if score_rows is None:
                out.append(list(zip(predictions[start:start + len(boxes)], boxes)))
            else:
                out.append(list(zip(predictions[start:start + len(boxes)], boxes, columns[1][start:start + len(boxes)])))
            start += len(boxes)
        return out
