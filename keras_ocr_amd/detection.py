"""Host-side mirror of ``keras_ocr.detection.Detector`` (reference ``keras_ocr/detection.py:661-785``).
The Keras model and the OpenCV post-processing are replaced by libkocr (HIP, gfx950)."""
import itertools
import typing

import numpy as np

from . import _lib, layout as _layout, tools, weights as _weights

PRETRAINED_WEIGHTS = {  # detection.py:647-658
    ("clovaai_general", True): {
        "url": "https://github.com/faustomorales/keras-ocr/releases/download/v0.8.4/craft_mlt_25k.pth",
        "filename": "craft_mlt_25k.pth",
        "sha256": "4a5efbfb48b4081100544e75e1e2b57f8de3d84f213004b14b85fd4b3748db17",
    },
    ("clovaai_general", False): {
        "url": "https://github.com/faustomorales/keras-ocr/releases/download/v0.8.4/craft_mlt_25k.h5",
        "filename": "craft_mlt_25k.h5",
        "sha256": "7283ce2ff05a0617e9740c316175ff3bacdd7215dbdf1a726890d5099431f899",
    },
}


def load_torch_state_dict(weights_path):
    """load_torch_weights' reader (detection.py:428-468): PyTorch state dict -> name -> ndarray."""
    import torch

    pretrained = torch.load(weights_path, map_location=torch.device("cpu"))
    return {k: v.numpy() for k, v in pretrained.items() if k.split(".")[-1] != "num_batches_tracked"}


def compute_input(image):
    """detection.compute_input (detection.py:34-42): RGB -> the network's normalised float32 input."""
    image = image.astype("float32")
    mean = np.array([0.485, 0.456, 0.406])
    variance = np.array([0.229, 0.224, 0.225])
    image -= mean * 255
    image /= variance * 255
    return image


def invert_input(X):  # pylint: disable=invalid-name
    """detection.invert_input (detection.py:45-52): compute_input's inverse, clipped to uint8."""
    X = X.copy()
    mean = np.array([0.485, 0.456, 0.406])
    variance = np.array([0.229, 0.224, 0.225])
    X *= variance * 255
    X += mean * 255
    return X.clip(0, 255).astype("uint8")


def get_gaussian_heatmap(size=512, distanceRatio=3.34):  # pylint: disable=invalid-name
    """detection.get_gaussian_heatmap (detection.py:55-62): the uint8 Gaussian compute_maps warps onto every character."""
    v = np.abs(np.linspace(-size / 2, size / 2, num=size))
    x, y = np.meshgrid(v, v)
    g = np.sqrt(x**2 + y**2)
    g *= distanceRatio / (size / 2)
    g = np.exp(-(1 / 2) * (g**2))
    g *= 255
    return g.clip(0, 255).astype("uint8")


def compute_maps(heatmap, image_height, image_width, lines):
    """detection.compute_maps (detection.py:106-198) on the default context: the CRAFT targets of one page, (H/2, W/2, 2)
    float32, region (text) map then affinity (link) map.  ``lines``: a list of lines, each a list of (points (4, 2),
    character).  Runs on the GPU (kocr_compute_maps), bit for bit the reference's full-map warps.
    Only a 2-D uint8 heat-map is supported."""
    heatmap = np.asarray(heatmap)
    if heatmap.dtype != np.uint8 or heatmap.ndim != 2:
        raise NotImplementedError(f"compute_maps supports a 2-D uint8 heat-map only, got {heatmap.dtype} of shape {heatmap.shape}")
    return _lib.default_context().compute_maps(heatmap, image_height, image_width, [lines])[0]


def map_to_rgb(y):
    """detection.map_to_rgb (detection.py:201-204): (h, w, 2) maps -> (h, w, 3) uint8 for display."""
    return (np.concatenate([y, np.zeros((y.shape[0], y.shape[1], 1))], axis=-1) * 255).astype("uint8")


def getBoxes(y_pred, detection_threshold=0.7, text_threshold=0.4, link_threshold=0.4, size_threshold=10,  # pylint: disable=invalid-name
             min_area_rect=None, return_scores=False):
    """detection.getBoxes (detection.py:207-287) on the default context: (N,h,w,2) float32 heat-maps -> list of (n_i,4,2)
    float32 boxes (``np.array([])`` for an image without boxes).  ``return_scores=True``: ``(box_groups, score_groups)``,
    per image an (n_i,) float32 array of detection scores -- the maximum of the text map over each box's component, the
    number compared with ``detection_threshold`` (detection.py:240).

    ``min_area_rect`` picks how ``cv2.boxPoints(cv2.minAreaRect(contour))`` (detection.py:273) is computed:
    ``"exact"`` -- the min-area rectangle in exact arithmetic (the default); ``"opencv"`` -- OpenCV's own float32 rotating
    calipers and ``RotatedRect::points`` (include/kocr.h: KOCR_RECT_OPENCV); ``None`` -- the context's rule
    (``Context.set_min_area_rect``)."""
    return _lib.default_context().get_boxes(y_pred, detection_threshold=detection_threshold, text_threshold=text_threshold,
                                            link_threshold=link_threshold, size_threshold=size_threshold,
                                            min_area_rect=min_area_rect, return_scores=return_scores)


def get_char_boxes(y_pred, box_groups, ctx=None, **rule):
    """The character boxes of word boxes, read off the region map the detector wrote (channel 0 of ``y_pred``) on the GPU
    (kocr_char_boxes; DESIGN.md section 4, "Characters"; the reference has no counterpart): ``y_pred`` (N,h,w,2) float32
    heat-maps, ``box_groups`` what ``getBoxes(y_pred)`` returned.  Returns, per image, one ``layout.Characters(boxes
    (K,4,2), scores (K,))`` per word box, in detector-input pixels like the boxes.  ``ctx``: a ``Context`` (None: the default
    one).  ``rule``: ``peak_threshold`` (default 0.4), ``valley_ratio`` (0.7), ``extent_threshold`` (0.2); the defaults are
    judgement, not fitted to real text.  The profile runs along tl -> tr: vertical text gives slices of the word; characters
    whose blobs merge come out as one box."""
    unknown = set(rule) - set(_lib.CHAR_RULE_DEFAULTS)
    if unknown:
        raise TypeError(f"get_char_boxes: unknown rule parameter(s) {sorted(unknown)}")
    context = _lib.default_context() if ctx is None or ctx is True else ctx
    return _layout.characters_of(context.char_boxes(y_pred, box_groups, **rule))


class _CraftModel:
    """Stands in for ``detector.model`` (inner seam #1): ``predict(X) -> heat-maps``."""

    def __init__(self, ctx):
        self._ctx = ctx
        self.input_shape = (None, None, None, 3)

    def predict(self, X, batch_size=32, **kwargs):  # pylint: disable=invalid-name,unused-argument
        return self._ctx.craft_forward(np.asarray(X), micro_batch=batch_size or 0)

    def evaluate(self, x, y, batch_size=None, sample_weight=None, **kwargs):  # pylint: disable=unused-argument
        """The loss of ``model.compile(loss="mse")`` (detection.py:696) as Keras' evaluate reports it: per pixel
        l = mean over the two maps of (y - y_hat)^2; with SUM_OVER_BATCH_SIZE and batch averages weighted by batch size
        this is sum_n w_n sum_p l_np / (N h w) whatever ``batch_size``.  The forward and the
        per-image sums run on the GPU (kocr_craft_mse); ``batch_size`` is the forward's micro-batch."""
        x = np.asarray(x)
        sums = self._ctx.craft_mse(x, y, micro_batch=batch_size or 0)
        n, h, w = np.shape(y)[:3]
        sw = np.ones(n) if sample_weight is None else np.asarray(sample_weight, np.float64).reshape(n)
        return float((sw * sums).sum() / (n * h * w))

    def fit(self, *args, **kwargs):
        """Training is not implemented (gradients are out of scope)."""
        raise NotImplementedError(_INFERENCE_ONLY)

    def compile(self, *args, **kwargs):
        """Training is not implemented (gradients are out of scope)."""
        raise NotImplementedError(_INFERENCE_ONLY)


_INFERENCE_ONLY = "keras-ocr_amd is inference-only: training (fit / compile) is not implemented"


class Detector:
    """A text detector using the CRAFT architecture (detection.py:661-696).

    Args:
        weights: ``"clovaai_general"`` (pretrained file looked up in / downloaded to the keras-ocr
            cache directory), ``None`` (random initialisation: the seeded synthetic weights of
            ``keras_ocr_amd.weights``), or a ``dict`` of state-dict arrays.
        load_from_torch: read ``craft_mlt_25k.pth`` instead of the Keras ``.h5``.
        optimizer: accepted for signature compatibility (inference only).
        backbone_name: only ``"vgg"``.
    """

    def __init__(self, weights="clovaai_general", load_from_torch=False, optimizer="adam", backbone_name="vgg",
                 ctx=None):
        del optimizer
        if backbone_name != "vgg":
            raise NotImplementedError("keras-ocr_amd implements the VGG backbone only.")
        self._ctx = ctx or _lib.default_context()
        if isinstance(weights, dict):
            state = weights
        elif weights is not None:
            pretrained_key = (weights, load_from_torch)
            assert pretrained_key in PRETRAINED_WEIGHTS, "Selected weights configuration not found."
            cfg = PRETRAINED_WEIGHTS[pretrained_key]
            path = tools.download_and_verify(url=cfg["url"], filename=cfg["filename"], sha256=cfg["sha256"])
            if path.endswith(".pth"):
                state = load_torch_state_dict(path)
            else:
                state = _weights.read_keras_h5(path, kind="craft")
        else:
            state = _weights.synthetic_craft_weights()
        self._ctx.load_craft(state)
        self.model = _CraftModel(self._ctx)

    def get_batch_generator(self, image_generator, batch_size=8, heatmap_size=512, heatmap_distance_ratio=1.5):
        """Detector.get_batch_generator (detection.py:698-743): batches (X, y) or, when the samples are
        (image, lines, sample_weight), (X, y, sample_weights) -- X = compute_input(images), y the compute_maps targets of
        every page, computed on the GPU in one call per batch.  Unlike the reference, an exhausted generator ends the
        iteration, and a last batch shorter than batch_size is yielded."""
        heatmap = get_gaussian_heatmap(size=heatmap_size, distanceRatio=heatmap_distance_ratio)
        while True:
            batch = list(itertools.islice(image_generator, batch_size))
            if not batch:
                return
            images = np.array([entry[0] for entry in batch])
            line_groups = [entry[1] for entry in batch]
            X = compute_input(images)  # pylint: disable=invalid-name
            y = self._ctx.compute_maps(heatmap, images.shape[1], images.shape[2], line_groups)
            if len(batch[0]) == 3:
                yield X, y, np.array([sample[2] for sample in batch])
            else:
                yield X, y

    def detect(self, images: typing.List[typing.Union[np.ndarray, str]], detection_threshold=0.7, text_threshold=0.4,
               link_threshold=0.4, size_threshold=10, min_area_rect=None, return_scores=False, char_boxes=None, **kwargs):
        """Detector.detect (detection.py:745-785): list/array of same-sized HxWx3 RGB images (or
        paths) -> list of (n_i,4,2) float32 box arrays.  ``min_area_rect``: ``"exact"`` / ``"opencv"`` for this
        call (see ``getBoxes``), ``None`` = the context's rule.  ``return_scores=True``: ``(box_groups, score_groups)`` as
        ``getBoxes``.  ``char_boxes`` (True, or a dict of ``get_char_boxes``' rule parameters): a last element
        ``char_groups``, per image one ``layout.Characters`` per box as ``get_char_boxes`` gives them, computed in the same
        call from the heat-maps in HBM -- ``(box_groups, char_groups)`` without scores."""
        images = [tools.read(image) for image in images]
        want_chars = _lib.char_rule(char_boxes) is not None
        if not images:
            return ([],) * (1 + bool(return_scores) + want_chars) if return_scores or want_chars else []
        batch = np.stack([np.asarray(im) for im in images])
        if batch.dtype != np.uint8:
            # the reference normalises whatever it is given (detection.py:34-42)
            mean = np.array([0.485, 0.456, 0.406])
            variance = np.array([0.229, 0.224, 0.225])
            batch = batch.astype("float32")
            batch -= mean * 255
            batch /= variance * 255
        out = self._ctx._detect(batch, detection_threshold, text_threshold, link_threshold, size_threshold,  # pylint: disable=protected-access
                                kwargs.get("batch_size", 0) or 0, None, min_area_rect, return_scores, char_boxes)
        if want_chars:
            out.characters = _layout.characters_of(out.characters)
        return out.render_detection()

    def detect_tiled(self, images, tile=1024, overlap=128, detection_threshold=0.7, text_threshold=0.4, link_threshold=0.4,
                     size_threshold=10, min_area_rect=None, return_scores=False, char_boxes=None, **kwargs):
        """``detect`` for pages larger than the detector takes in one image ("Tiled pages"): every page
        is padded with 255 (``tools.pad``) to the canvas of ``tools.tile_plan(height, width, tile, overlap)``, the detector
        runs on its overlapping tiles, ``batch_size`` tiles at a time, and getBoxes on the heat-map stitched from the tiles'
        cores in HBM.  Same-sized uint8 images (NotImplementedError otherwise); every other argument and the return value
        as ``detect``.  Pixels nearer than the detector's receptive field to a tile edge differ from a whole-page pass."""
        images = [tools.read(image) for image in images]
        want_chars = _lib.char_rule(char_boxes) is not None
        if not images:
            return ([],) * (1 + bool(return_scores) + want_chars) if return_scores or want_chars else []
        batch = np.stack([np.asarray(im) for im in images])
        if batch.dtype != np.uint8:
            raise NotImplementedError("detect_tiled: only uint8 images are read in tiles (the tile copy moves RGB bytes)")
        plan = tools.tile_plan(batch.shape[1], batch.shape[2], tile, overlap)
        canvas = np.stack([tools.pad(im, width=plan.canvas[1], height=plan.canvas[0]) for im in batch])
        out = self._ctx._detect_tiled(canvas, tile, overlap, detection_threshold, text_threshold, link_threshold,  # pylint: disable=protected-access
                                      size_threshold, kwargs.get("batch_size", 0) or 0, None, min_area_rect, return_scores, char_boxes)
        if want_chars:
            out.characters = _layout.characters_of(out.characters)
        return out.render_detection()
