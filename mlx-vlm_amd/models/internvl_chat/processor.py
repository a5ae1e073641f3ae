"""InternVL processor - host mirror of the reference's `mlx_vlm/models/internvl_chat/processor.py`: `dynamic_preprocess`
(82-158: the tile grid whose aspect ratio is closest to the image's among all grids of min_num .. max_num tiles, ties to the
grid closer in area; bicubic resize to the grid, row-major crops, a thumbnail behind a split image), `build_transform` (24-58:
bicubic resize to the tile, / 255, ImageNet mean / std in float32), InternVLImageProcessor (161-261), InternVLChatProcessor
(264-461: `<image>` -> `<img>` + `<IMG_CONTEXT>` x (tokens per tile x tiles) + `</img>`, left padding, `image_token_index` handed on).
Host code (PIL + numpy); pixel values are float32 [tiles, 3, size, size]."""
from __future__ import annotations

import json
import os
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
IMG_START_TOKEN, IMG_END_TOKEN, IMG_CONTEXT_TOKEN = "<img>", "</img>", "<IMG_CONTEXT>"


def target_ratios(min_num: int, max_num: int) -> List[Tuple[int, int]]:
    """every (columns, rows) grid of min_num .. max_num tiles, sorted by tile count; grids of equal count keep the iteration order
    of the set they are collected in, which is the reference's own construction (the order decides ties)"""
    s = set((i, j) for n in range(min_num, max_num + 1) for i in range(1, n + 1) for j in range(1, n + 1)
            if min_num <= i * j <= max_num)
    return sorted(s, key=lambda x: x[0] * x[1])


def find_closest_aspect_ratio(aspect_ratio, ratios, width, height, image_size):
    best_diff, best = float("inf"), (1, 1)
    area = width * height
    for r in ratios:
        diff = abs(aspect_ratio - r[0] / r[1])
        if diff < best_diff:
            best_diff, best = diff, r
        elif diff == best_diff:
            if abs(area - image_size * image_size * r[0] * r[1]) < abs(area - image_size * image_size * best[0] * best[1]):
                best = r
    return best


def tile_plan(width: int, height: int, min_num=1, max_num=12, image_size=448, use_thumbnail=False, ratios=None):
    """-> ((columns, rows), crop boxes (left, top, right, bottom) in the resized image, thumbnail appended?)"""
    if width == 0 or height == 0:
        return (0, 0), [], False
    grid = find_closest_aspect_ratio(width / height, ratios if ratios is not None else target_ratios(min_num, max_num), width,
                                     height, image_size)
    blocks = grid[0] * grid[1]
    boxes = [((i % grid[0]) * image_size, (i // grid[0]) * image_size, (i % grid[0] + 1) * image_size,
              (i // grid[0] + 1) * image_size) for i in range(blocks)]
    return grid, boxes, bool(use_thumbnail and blocks > 1)


def dynamic_preprocess(image, min_num=1, max_num=12, image_size=448, use_thumbnail=False, ratios=None):
    """-> list of PIL tiles (image_size x image_size)"""
    from PIL import Image

    w, h = image.size
    grid, boxes, thumb = tile_plan(w, h, min_num, max_num, image_size, use_thumbnail, ratios)
    if not boxes:
        return []
    resized = image.resize((image_size * grid[0], image_size * grid[1]), resample=Image.Resampling.BICUBIC)
    tiles = [resized.crop(b) for b in boxes]
    if thumb:
        tiles.append(image.resize((image_size, image_size), resample=Image.Resampling.BICUBIC))
    return tiles


def transform(img, input_size: int, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
    """build_transform's function -> float32 [3, input_size, input_size]"""
    from PIL import Image

    if img.mode != "RGB":
        img = img.convert("RGB")
    img = img.resize((input_size, input_size), resample=Image.Resampling.BICUBIC)
    x = np.array(img).astype(np.float32) / np.float32(255.0)
    x = x.transpose(2, 0, 1)
    m = np.asarray(mean, dtype=np.float64).astype(np.float32)[:, None, None]
    s = np.asarray(std, dtype=np.float64).astype(np.float32)[:, None, None]
    return ((x - m) / s).astype(np.float32)


def _to_pil(im):
    from PIL import Image

    if isinstance(im, Image.Image):
        return im
    a = np.asarray(im)
    if a.ndim == 3 and a.shape[0] in (1, 3) and a.shape[-1] not in (1, 3):
        a = a.transpose(1, 2, 0)
    return Image.fromarray(a.astype(np.uint8)).convert("RGB")


class InternVLImageProcessor:
    model_input_names = ["pixel_values"]

    def __init__(self, size: int = 448, image_mean=IMAGENET_MEAN, image_std=IMAGENET_STD, do_dynamic_preprocess: bool = True,
                 dynamic_min_num: int = 1, dynamic_max_num: int = 12, dynamic_use_thumbnail: bool = True, **kwargs):
        self.size = int(size)
        self.image_mean, self.image_std = tuple(image_mean), tuple(image_std)
        self.do_dynamic_preprocess = do_dynamic_preprocess
        self.dynamic_min_num, self.dynamic_max_num = int(dynamic_min_num), int(dynamic_max_num)
        self.dynamic_use_thumbnail = bool(dynamic_use_thumbnail)
        self._ratios = target_ratios(self.dynamic_min_num, self.dynamic_max_num)

    def preprocess(self, images, do_dynamic_preprocess: Optional[bool] = None, size: Optional[int] = None, **kwargs):
        """-> {"pixel_values": float32 [1, total tiles, 3, size, size], "num_patches_list": tiles per image}"""
        dyn = self.do_dynamic_preprocess if do_dynamic_preprocess is None else do_dynamic_preprocess
        size = self.size if size is None else int(size)
        if not isinstance(images, (list, tuple)):
            images = [images]
        per_image = []
        for im in images:
            im = _to_pil(im)
            if dyn:
                tiles = dynamic_preprocess(im, self.dynamic_min_num, self.dynamic_max_num, size, self.dynamic_use_thumbnail,
                                           self._ratios if size == self.size else None)
            else:
                from PIL import Image

                tiles = [im.resize((size, size), resample=Image.Resampling.BICUBIC)]
            per_image.append(np.stack([transform(t, size, self.image_mean, self.image_std) for t in tiles]))
        return {"pixel_values": np.concatenate(per_image, axis=0)[None], "num_patches_list": [p.shape[0] for p in per_image]}

    __call__ = preprocess


class InternVLChatProcessor:
    def __init__(self, image_processor=None, tokenizer=None, chat_template: Optional[str] = None, num_image_token=None,
                 image_size: int = 448, patch_size: int = 14, downsample_ratio: float = 0.5, **kwargs):
        self.image_processor = image_processor or InternVLImageProcessor(**kwargs)
        self.tokenizer = tokenizer
        self.chat_template = chat_template if chat_template is not None else getattr(tokenizer, "chat_template", None)
        self.num_image_token = int(num_image_token) if num_image_token is not None else \
            int((image_size // patch_size) ** 2 * (downsample_ratio ** 2))
        self.image_token = "<image>"
        self.img_context_token_id = tokenizer.convert_tokens_to_ids(IMG_CONTEXT_TOKEN) if tokenizer is not None else None

    def image_tokens(self, n_tiles: int) -> str:
        return IMG_START_TOKEN + IMG_CONTEXT_TOKEN * self.num_image_token * n_tiles + IMG_END_TOKEN

    def expand_prompts(self, text: Sequence[str], n_images: int, num_patches_list: Sequence[int]) -> List[str]:
        """reference processor.py:324-361"""
        tiles = lambda i: num_patches_list[i] if i < len(num_patches_list) else 1       # noqa: E731
        if n_images >= 1 and len(text) == 1:
            q = text[0]
            missing = n_images - q.count("<image>")
            if missing > 0:
                q = "<image>\n" * missing + q
            for i in range(n_images):
                q = q.replace("<image>", self.image_tokens(tiles(i)), 1)
            return [q]
        out = []
        for i in range(n_images):
            q = text[i]
            if "<image>" not in q:
                q = "<image>\n" + q
            out.append(q.replace("<image>", self.image_tokens(tiles(i)), 1))
        return out

    def __call__(self, text: Union[str, List[str], None] = None, images=None, padding=True, **kwargs):
        kwargs.pop("return_tensors", None)
        if kwargs.get("videos") is not None:
            raise NotImplementedError("video inputs are outside the built hot path")
        out = {}
        texts = None if text is None else ([text] if isinstance(text, str) else list(text))
        feats = None
        if images is not None and (not isinstance(images, (list, tuple)) or len(images)):
            images = list(images) if isinstance(images, (list, tuple)) else [images]
            feats = self.image_processor.preprocess(images)
            out["pixel_values"] = feats["pixel_values"][0]                               # [tiles, 3, S, S]
        if texts is not None:
            queries = self.expand_prompts(texts, len(images), feats["num_patches_list"]) if feats is not None else texts
            self.tokenizer.padding_side = "left"
            enc = self.tokenizer(queries, padding=padding)
            out["input_ids"] = np.asarray(enc["input_ids"], dtype=np.int64)
            out["attention_mask"] = np.asarray(enc["attention_mask"], dtype=np.int32)
        out["image_token_index"] = self.img_context_token_id
        return out

    def decode(self, *a, **k):
        return self.tokenizer.decode(*a, **k)

    def batch_decode(self, *a, **k):
        return self.tokenizer.batch_decode(*a, **k)

    @classmethod
    def from_pretrained(cls, model_path: str, tokenizer=None, **kwargs):
        """reference processor.py:394-461: tile geometry from config.json (`force_image_size` over vision_config.image_size,
        `max_dynamic_patch`, `min_dynamic_patch`, `use_thumbnail`, `downsample_ratio`), overridden by processor_config.json"""
        if tokenizer is None:
            from transformers import AutoTokenizer

            tokenizer = AutoTokenizer.from_pretrained(model_path)
        image_size, patch_size, ratio, max_n, min_n, thumb = 448, 14, 0.5, 12, 1, True
        cp = os.path.join(model_path, "config.json")
        if os.path.exists(cp):
            with open(cp) as f:
                c = json.load(f)
            vc = c.get("vision_config", {}) or {}
            image_size = c.get("force_image_size", vc.get("image_size", 448))
            patch_size = vc.get("patch_size", 14)
            ratio = c.get("downsample_ratio", 0.5)
            max_n, min_n, thumb = c.get("max_dynamic_patch", 12), c.get("min_dynamic_patch", 1), c.get("use_thumbnail", True)
        pk = {}
        pp = os.path.join(model_path, "processor_config.json")
        if os.path.exists(pp):
            with open(pp) as f:
                pc = json.load(f)
            pk = {k: pc[k] for k in ("num_image_token", "image_size", "patch_size", "downsample_ratio") if k in pc}
        image_size, patch_size, ratio = pk.pop("image_size", image_size), pk.pop("patch_size", patch_size), pk.pop("downsample_ratio", ratio)
        first = lambda v: v[0] if isinstance(v, (list, tuple)) else v                    # noqa: E731
        image_size, patch_size = int(first(image_size)), int(first(patch_size))
        ip = InternVLImageProcessor(size=image_size, dynamic_max_num=max_n, dynamic_min_num=min_n, dynamic_use_thumbnail=thumb)
        return cls(image_processor=ip, tokenizer=tokenizer, image_size=image_size, patch_size=patch_size, downsample_ratio=ratio, **pk)
