"""``renderers.plan_volume``: the one host-side decision on which render-ready copy of the volume a forward marches.

ROWS was recorded from the code before the planner existed (commit 46eb5ba): its ``_use_ypairs`` / ``_use_bricks`` predicates and the
``if`` chains of ``_Render.forward`` + ``render()`` (rows without ``static``; checked equal to ``_RenderFromCamera.forward``'s chain
on every row without a mask) and of ``RegistrationStage._bind_volume`` (``static`` rows), run over inputs at the edges of every
condition.  A row is (inputs that differ from DEFAULT, (kind, layout, first_sight, labels_in_taps, hu_in_pack)); ``first_sight``
was recorded as "the copy is built at the first render of a volume version", i.e. forced or with a LAYOUT_COPY_AFTER count of 0.
n = 64 * wavefronts at B = 1.  The planner must reproduce every row."""
import contextlib

import pytest
import torch

from xvr_amd import _lib, renderers
from xvr_amd.renderers import VolumePlan, plan_volume
from xvr_amd.spec import RenderSpec

DEFAULT = dict(spec={}, shape=(64, 64, 64), B=1, n=2048 * 64, C=1, storage="float32", masked=False, aligned=True, contiguous=True,
               lazy_hu=False, static=False)
# every knob and option the planner reads, at its default: a row does not depend on the environment or on an earlier test
KNOBS = dict(YPAIR_LAYOUT=True, YPAIR_TILES=True, YPAIR_TILES_PACKED=True, YPAIR_MIN_WAVEFRONTS=2048,
             YPAIR_FIRST_SIGHT_SAMPLES_PER_VOXEL=10.0, BRICK_LAYOUT=True, BRICK_NX=True, PACK_LABELS=True,
             LAYOUT_COPY_AFTER={"ypairs": 2, "bricks": 0, "htiles": 0})
OPTIONS = dict(siddon_slab=1, fwd_split=0)

ROWS = [
    ({'spec': {'renderer': 'trilinear'}, 'B': 1, 'n': 131008}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'B': 1, 'n': 131072}, ('ypairs', 3, True, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'B': 1, 'n': 131073}, ('ypairs', 3, True, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'B': 23, 'n': 5696}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'B': 2, 'n': 65473}, ('ypairs', 3, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'B': 1, 'n': 131008}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'B': 1, 'n': 131072}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'B': 1, 'n': 131073}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'B': 23, 'n': 5696}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'B': 2, 'n': 65473}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'B': 1, 'n': 131008}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'B': 1, 'n': 131072}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'B': 1, 'n': 131073}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'B': 23, 'n': 5696}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'B': 2, 'n': 65473}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'B': 1, 'n': 131008}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'B': 1, 'n': 131072}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'B': 1, 'n': 131073}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'B': 23, 'n': 5696}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'B': 2, 'n': 65473}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': -1}, 'n': 262144}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'shape': (4, 4, 8191), 'knobs': {'YPAIR_TILES': True}}, ('ypairs', 3, True, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'shape': (4, 4, 8192), 'knobs': {'YPAIR_TILES': True}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'shape': (4, 4, 8191), 'knobs': {'YPAIR_TILES': False}}, ('ypairs', 1, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'shape': (4, 4, 8192), 'knobs': {'YPAIR_TILES': False}}, ('ypairs', 1, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'shape': (1, 64, 64)}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'shape': (2, 64, 64)}, ('ypairs', 3, True, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'shape': (64, 64, 1)}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'shape': (1, 64, 64)}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'shape': (2, 64, 64)}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'shape': (64, 64, 1)}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'shape': (2048, 1023, 442)}, ('ypairs', 3, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'shape': (2048, 1023, 443)}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'shape': (1024, 1023, 1023), 'knobs': {'YPAIR_TILES': False}}, ('ypairs', 1, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'shape': (1024, 1023, 1024), 'knobs': {'YPAIR_TILES': False}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'shape': (2048, 2048, 504)}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'shape': (2048, 2048, 512)}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 1, 'masked': True}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 2, 'masked': False}, ('ypairs', 3, True, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 2, 'masked': True}, ('packed_ypairs', 3, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 16, 'masked': False}, ('ypairs', 3, True, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 16, 'masked': True}, ('packed_ypairs', 3, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 17, 'masked': False}, ('ypairs', 3, True, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 17, 'masked': True}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 1, 'masked': False}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 1, 'masked': True}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 2, 'masked': False}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 2, 'masked': True}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 16, 'masked': False}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 16, 'masked': True}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 17, 'masked': False}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 17, 'masked': True}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131072, 'C': 1, 'masked': True}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131072, 'C': 2, 'masked': False}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131072, 'C': 2, 'masked': True}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131072, 'C': 16, 'masked': False}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131072, 'C': 16, 'masked': True}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131072, 'C': 17, 'masked': False}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131072, 'C': 17, 'masked': True}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 6400, 'C': 1, 'masked': False}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 6400, 'C': 1, 'masked': True}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 6400, 'C': 2, 'masked': False}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 6400, 'C': 2, 'masked': True}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 6400, 'C': 16, 'masked': False}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 6400, 'C': 16, 'masked': True}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 6400, 'C': 17, 'masked': False}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 6400, 'C': 17, 'masked': True}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 3, 'masked': True, 'lazy_hu': False}, ('packed_ypairs', 3, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 3, 'masked': True, 'lazy_hu': False, 'aligned': False}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 3, 'masked': True, 'lazy_hu': False, 'contiguous': False}, ('packed_ypairs', 3, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 3, 'masked': True, 'lazy_hu': False, 'knobs': {'PACK_LABELS': False}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 3, 'masked': True, 'lazy_hu': False, 'knobs': {'YPAIR_TILES_PACKED': False}}, ('packed_ypairs', 1, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 3, 'masked': True, 'lazy_hu': False, 'knobs': {'YPAIR_TILES': False}}, ('packed_ypairs', 1, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 3, 'masked': True, 'lazy_hu': False, 'knobs': {'YPAIR_LAYOUT': False}}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 3, 'masked': True, 'lazy_hu': True}, ('packed_ypairs', 3, True, True, True)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 3, 'masked': True, 'lazy_hu': True, 'aligned': False}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 3, 'masked': True, 'lazy_hu': True, 'contiguous': False}, ('packed_ypairs', 3, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 3, 'masked': True, 'lazy_hu': True, 'knobs': {'PACK_LABELS': False}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 3, 'masked': True, 'lazy_hu': True, 'knobs': {'YPAIR_TILES_PACKED': False}}, ('packed_ypairs', 1, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 3, 'masked': True, 'lazy_hu': True, 'knobs': {'YPAIR_TILES': False}}, ('packed_ypairs', 1, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 131072, 'C': 3, 'masked': True, 'lazy_hu': True, 'knobs': {'YPAIR_LAYOUT': False}}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 3, 'masked': True, 'lazy_hu': False}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 3, 'masked': True, 'lazy_hu': False, 'aligned': False}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 3, 'masked': True, 'lazy_hu': False, 'contiguous': False}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 3, 'masked': True, 'lazy_hu': False, 'knobs': {'PACK_LABELS': False}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 3, 'masked': True, 'lazy_hu': False, 'knobs': {'YPAIR_TILES_PACKED': False}}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 3, 'masked': True, 'lazy_hu': False, 'knobs': {'YPAIR_TILES': False}}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 3, 'masked': True, 'lazy_hu': False, 'knobs': {'YPAIR_LAYOUT': False}}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 3, 'masked': True, 'lazy_hu': True}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 3, 'masked': True, 'lazy_hu': True, 'aligned': False}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 3, 'masked': True, 'lazy_hu': True, 'contiguous': False}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 3, 'masked': True, 'lazy_hu': True, 'knobs': {'PACK_LABELS': False}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 3, 'masked': True, 'lazy_hu': True, 'knobs': {'YPAIR_TILES_PACKED': False}}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 3, 'masked': True, 'lazy_hu': True, 'knobs': {'YPAIR_TILES': False}}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'C': 3, 'masked': True, 'lazy_hu': True, 'knobs': {'YPAIR_LAYOUT': False}}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'C': 17, 'masked': True, 'lazy_hu': True}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'lazy_hu': True}, ('ypairs', 3, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'C': 3, 'masked': True, 'lazy_hu': True}, ('packed', 0, True, True, False)),
    ({'spec': {'renderer': 'trilinear'}, 'knobs': {'YPAIR_TILES_PACKED': False}}, ('ypairs', 3, True, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'knobs': {'YPAIR_TILES': False}}, ('ypairs', 1, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'knobs': {'YPAIR_LAYOUT': False}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'knobs': {'BRICK_LAYOUT': False}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'knobs': {'YPAIR_MIN_WAVEFRONTS': 1}}, ('ypairs', 3, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 6400, 'knobs': {'YPAIR_MIN_WAVEFRONTS': 1}}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 64, 'knobs': {'YPAIR_MIN_WAVEFRONTS': 1}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 128, 'knobs': {'YPAIR_MIN_WAVEFRONTS': 1}}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'storage': 'float16', 'static': False}, ('htiles', 4, True, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 6400, 'storage': 'float16', 'static': True}, ('htiles', 4, True, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 262144, 'storage': 'float16', 'static': False}, ('htiles', 4, True, False, False)),
    ({'spec': {'renderer': 'trilinear'}, 'n': 262144, 'storage': 'float16', 'static': True}, ('htiles', 4, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131136, 'options': {'siddon_slab': 0, 'fwd_split': 0}}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131136, 'options': {'siddon_slab': 0, 'fwd_split': 1}}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131136, 'options': {'siddon_slab': 0, 'fwd_split': 2}}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131136, 'options': {'siddon_slab': 1, 'fwd_split': 0}}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131136, 'options': {'siddon_slab': 1, 'fwd_split': 1}}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131136, 'options': {'siddon_slab': 1, 'fwd_split': 2}}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131136, 'shape': (2, 4096, 4095)}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131136, 'shape': (2, 4096, 4096)}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131136, 'shape': (511, 1024, 1024)}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131136, 'shape': (512, 1024, 1024)}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131136, 'shape': (2, 2, 12278)}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131136, 'shape': (2, 2, 12279)}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 131136, 'options': {'siddon_slab': 0, 'fwd_split': 0}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 131136, 'options': {'siddon_slab': 0, 'fwd_split': 1}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 131136, 'options': {'siddon_slab': 0, 'fwd_split': 2}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 131136, 'options': {'siddon_slab': 1, 'fwd_split': 0}}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 131136, 'options': {'siddon_slab': 1, 'fwd_split': 1}}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 131136, 'options': {'siddon_slab': 1, 'fwd_split': 2}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 131136, 'shape': (2, 4096, 4095)}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 131136, 'shape': (2, 4096, 4096)}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 131136, 'shape': (511, 1024, 1024)}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 131136, 'shape': (512, 1024, 1024)}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 131136, 'shape': (2, 2, 12278)}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 131136, 'shape': (2, 2, 12279)}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'n': 131136, 'options': {'siddon_slab': 0, 'fwd_split': 0}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'n': 131136, 'options': {'siddon_slab': 0, 'fwd_split': 1}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'n': 131136, 'options': {'siddon_slab': 0, 'fwd_split': 2}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'n': 131136, 'options': {'siddon_slab': 1, 'fwd_split': 0}}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'n': 131136, 'options': {'siddon_slab': 1, 'fwd_split': 1}}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'n': 131136, 'options': {'siddon_slab': 1, 'fwd_split': 2}}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'n': 131136, 'shape': (2, 4096, 4095)}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'n': 131136, 'shape': (2, 4096, 4096)}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'n': 131136, 'shape': (511, 1024, 1024)}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'n': 131136, 'shape': (512, 1024, 1024)}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'n': 131136, 'shape': (2, 2, 12278)}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon', 'align_corners': True}, 'n': 131136, 'shape': (2, 2, 12279)}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear', 'n_points': 20}}, ('ypairs', 3, False, False, False)),
    ({'spec': {'renderer': 'trilinear', 'n_points': 20}, 'knobs': {'YPAIR_TILES': False}}, ('ypairs', 1, False, False, False)),
    ({'spec': {'renderer': 'trilinear', 'n_points': 21}}, ('ypairs', 3, True, False, False)),
    ({'spec': {'renderer': 'trilinear', 'n_points': 21}, 'knobs': {'YPAIR_TILES': False}}, ('ypairs', 1, False, False, False)),
    ({'spec': {'renderer': 'trilinear', 'n_points': 21}, 'knobs': {'YPAIR_FIRST_SIGHT_SAMPLES_PER_VOXEL': 11.0}}, ('ypairs', 3, False, False, False)),
    ({'spec': {'renderer': 'trilinear', 'n_points': 20}, 'knobs': {'YPAIR_FIRST_SIGHT_SAMPLES_PER_VOXEL': 9.5}}, ('ypairs', 3, True, False, False)),
    ({'spec': {'renderer': 'trilinear', 'n_points': 20}, 'knobs': {'LAYOUT_COPY_AFTER': {'ypairs': 0}}}, ('ypairs', 3, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'knobs': {'LAYOUT_COPY_AFTER': {'bricks': 2}}}, ('bricks', 2, False, False, False)),
    ({'spec': {'renderer': 'trilinear', 'n_points': 1}, 'n': 131072, 'static': True}, ('ypairs', 3, True, False, False)),
    ({'spec': {'renderer': 'trilinear', 'n_points': 1}, 'n': 6400, 'static': True}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 131072, 'static': True}, ('bricks', 2, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'n': 6400, 'static': True}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 131072, 'static': True}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'siddon', 'norm_dims_offset': 1}, 'n': 6400, 'static': True}, (None, 0, False, False, False)),
    ({'spec': {'renderer': 'trilinear', 'n_points': 1}, 'static': True, 'knobs': {'YPAIR_TILES': False}}, ('ypairs', 1, True, False, False)),
    ({'spec': {'renderer': 'siddon'}, 'static': True, 'knobs': {'LAYOUT_COPY_AFTER': {'bricks': 2}}}, ('bricks', 2, False, False, False)),
]


def _plan(row, monkeypatch):
    case = {**DEFAULT, **row}
    knobs, options = {**KNOBS, **case.pop("knobs", {})}, {**OPTIONS, **case.pop("options", {})}
    for name, value in knobs.items():
        if name == "LAYOUT_COPY_AFTER":
            for kind, count in {**KNOBS[name], **value}.items():
                monkeypatch.setitem(renderers.LAYOUT_COPY_AFTER, kind, count)
        else:
            monkeypatch.setattr(renderers, name, value)
    with contextlib.ExitStack() as stack:
        for name, value in options.items():
            stack.enter_context(_lib.option(name, value))      # (put back on exit)
        return plan_volume(RenderSpec(**case.pop("spec")), **case)


@pytest.mark.parametrize("row,expected", ROWS, ids=[f"{i}-{e[0]}" for i, (_, e) in enumerate(ROWS)])
def test_plan_is_the_decision_of_the_three_call_sites_it_replaced(row, expected, monkeypatch):
    plan = _plan(row, monkeypatch)
    assert isinstance(plan, VolumePlan) and tuple(plan) == expected, (row, plan)
    assert plan._fields == ("kind", "layout", "first_sight", "labels_in_taps", "hu_in_pack")
    with pytest.raises(AttributeError):
        plan.kind = "bricks"       # immutable


TRI, SID = {"renderer": "trilinear"}, {"renderer": "siddon"}
MASKED = dict(spec=TRI, C=3, masked=True)


@pytest.mark.parametrize("row,knob,expected", [
    (dict(spec=TRI), {"YPAIR_LAYOUT": False}, VolumePlan()),
    (dict(spec=TRI), {"YPAIR_TILES": False}, VolumePlan("ypairs", 1, False)),
    (MASKED, {"YPAIR_TILES_PACKED": False}, VolumePlan("packed_ypairs", 1, True, True)),
    (dict(spec=TRI), {"YPAIR_MIN_WAVEFRONTS": 2049}, VolumePlan()),
    (dict(spec=TRI), {"YPAIR_FIRST_SIGHT_SAMPLES_PER_VOXEL": float("inf")}, VolumePlan("ypairs", 3, False)),
    (dict(spec=SID), {"BRICK_LAYOUT": False}, VolumePlan()),
    (MASKED, {"PACK_LABELS": False}, VolumePlan()),
    (dict(spec=SID), {"LAYOUT_COPY_AFTER": {"bricks": 1}}, VolumePlan("bricks", 2, False)),
], ids=lambda v: next(iter(v)) if isinstance(v, dict) and next(iter(v)).isupper() else None)
def test_a_monkeypatched_knob_changes_the_plan(row, knob, expected, monkeypatch):
    """The knobs stay plain attributes of ``renderers`` read at call time: what the suite patches must still bite."""
    before = _plan(row, monkeypatch)
    after = _plan({**row, "knobs": knob}, monkeypatch)
    assert after == expected and after != before, (before, after)


@pytest.mark.gpu
@pytest.mark.parametrize("renderer,storage,kind", [("trilinear", "float32", "ypairs"), ("trilinear", "float16", "htiles"),
                                                   ("siddon", "float32", "bricks")])
def test_registration_stage_marches_the_copy_the_plan_names(renderer, storage, kind, monkeypatch):
    """The device-resident registration stage is the one site the suite pinned only through its images: the packing pass the plan
    names runs once per volume version -- at first sight, and once more after an in-place change -- and the stage's CSpec carries
    the plan's layout."""
    from xvr_amd.data import make_phantom, read
    from xvr_amd.drr import DRR
    from xvr_amd.pose import convert
    from xvr_amd.pose_opt import RegistrationStage
    from xvr_amd.similarity import FusedSimilarity

    vol, _ = make_phantom((30, 34, 38), n_ellipsoids=6, seed=5, device="cuda")
    kw = dict(spacing=(2.0, 2.0, 2.0), orientation="AP")
    with torch.no_grad():   # the target from a volume object of its own: nothing of `drr`'s is in the cache before the stage binds it
        target = DRR(read(vol.clone(), **kw), 1020.0, 32, 4.0, renderer=renderer, reverse_x_axis=False).cuda()(
            convert(torch.tensor([[3.10, 0.05, -0.03], [3.0, -0.05, 0.04]]).cuda(), torch.tensor([[4.0, 700.0, -6.0], [-3.0, 690.0, 5.0]]).cuda(),
                    parameterization="euler_angles", convention="ZXY"))
    extra = {"volume_storage": storage} if storage != "float32" else {}
    drr = DRR(read(vol, **kw), 1020.0, 32, 4.0, renderer=renderer, reverse_x_axis=False, **extra).cuda()
    rot, xyz = torch.tensor([[3.18, 0.0, 0.02], [3.05, 0.0, 0.0]]).cuda(), torch.tensor([[-6.0, 715.0, 5.0], [0.0, 700.0, 0.0]]).cuda()
    monkeypatch.setattr(renderers, "YPAIR_MIN_WAVEFRONTS", 1)
    monkeypatch.setattr(renderers, "PROFILER", [])
    stage = RegistrationStage(drr, FusedSimilarity(target.reshape(2, 1, 32, 32), per_image=True), rot, xyz, max_iters=16)
    plan = plan_volume(stage.rspec, tuple(drr.density.shape), 2, 32 * 32, storage=storage, static=True)
    assert plan.kind == kind and plan.first_sight
    stage.run(4, check_every=2, use_graph=False)
    names = [e[0] for e in renderers.PROFILER]
    assert names.count(f"pack_{kind}") == 1 and names.count(f"{renderer}_forward+jac") == 4, names
    assert stage.cspec.volume_layout == plan.layout != 0
    assert stage.vol_render is renderers._VOLUME_CACHE[id(drr.density)][kind][1]
    drr.density.mul_(0.5)
    stage.run(2, check_every=2, use_graph=False)
    names = [e[0] for e in renderers.PROFILER]
    assert names.count(f"pack_{kind}") == 2 and names.count(f"{renderer}_forward+jac") == 6, names
    assert stage.cspec.volume_layout == plan.layout
