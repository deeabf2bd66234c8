"""CBConv2d and its fused 1x1 tail (CBTail1x1): the change-based convolution module on MI355X.  (The pooling modules
live in pool.py; LazyPool, CBPoolMax2d and CBPoolAvg2d stay importable from here.)

Same torch.nn.Module surface as the reference (pycbinfer/conv2d.py): constructor arguments, the
attribute flags set from outside (threshold, withReLU, saveChangeMap, propChangeIndexes,
gatherComputationStats, finegrained, copyInput, feedbackLoop), the registered state buffers
(prevInput, prevOutput, outputState), clearMemory()/getStateTensors(), the
('changeIndexes', output, indexes) tuple protocol between modules, and the returned tensor aliasing
the layer state.  What differs is underneath: a frame of a layer is ONE call into libcbinfer_hip.so
that enqueues detection -> compaction -> fused gather/MFMA/scatter on torch's current stream with the
changed-pixel count kept on the device, so a whole network frame runs without a host round trip and
can be captured into a hipGraph (torch.cuda.CUDAGraph).

Two execution modes, chosen per module by `syncIndexes` (default False):
  False: sync-free.  Change lists travel as `ChangeIndexes` (capacity buffer + device count).
  True : like the reference, block on the count after compaction; change lists are exact IntTensors
         and the reference-structured op sequence (changeDetection, changeIndexesExtr, genXMatrix,
         matrixMult, updateOutput) of conv2d_cg.py is what runs.
"""
import contextlib
import ctypes
import functools
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import C, check, dtype_code, ptr, raw_stream, require_device, stream_ptr
from .conv2d_cg import (ChangeIndexes, MaskChangeIndexes, changeDetection, changeIndexesExtr, dilateChangeIndexes,
                        genXMatrix, matrixMult, newConvWorkspace, prepWeights, updateOutput)
from .conv2d_fg import cbconvFG, cbconvFG_deterministic
from .pool import CBPoolAvg2d, CBPoolMax2d, LazyPool      # noqa: F401  (the pools are re-exported: pickles name them here)


def _same_shape(t, shape):
    return t is not None and tuple(t.size()) == tuple(shape)


@functools.lru_cache(maxsize=None)
def _split_fits(Cin, K, kH, kW, H, W):
    """The shape-only part of the split-state tests: the library takes the layer, the frame mask fits its records."""
    return (bool(C.cbinfer_split_supported(Cin, K, kH, kW)) and
            C.cbinfer_mask_words(H, W) <= C.cbinfer_split_max_mask_words(K) and H * W * W < (1 << 32))


# Every CBINFER_* switch the Python package reads: name -> (default, what it does); a bool switch is on when set to '1'.
# They are read through _switch() when a frame takes the general path, so a test may flip one in mid-run; a call plan
# replayed instead looks only at the switches of its own path (the split-state plans: _split_switches()).
# CBINFER_NO_CHAIN is read once, at import; shard.py reads the last two itself.
SWITCHES = {
    'CBINFER_ARITH': ('x3', "fp32 split-state arithmetic: 'x3' (bf16 triples), 'f16x2'; else the list kernels"),
    'CBINFER_EXACT_F32': (False, "every fp32 layer on the exact f32 fma chain, as exactF32=True"),
    'CBINFER_NO_SPLIT': (False, "no split-state frames (fp32 and fp16)"),
    'CBINFER_NO_SPLIT_FG': (False, "no fine-grained frames on the split-state kernels"),
    'CBINFER_SPLIT_MINK': (0, "fewest output channels of an fp32 split-state layer"),
    'CBINFER_SPLIT_MAXK': (100000, "most output channels of an fp32 split-state layer"),
    'CBINFER_NO_HSPLIT': (False, "no fp16 split-state frames"),
    'CBINFER_HSPLIT_DEEP': (True, "fp16 split-state frames also for contractions of 48 k-stages and more"),
    'CBINFER_NO_SELFCOMPACT': (False, "no self-compacting frames: detection, compaction and contraction apart"),
    'CBINFER_NO_ROWCONV': (False, "no row-segment contraction (cb_rowconv.hip)"),
    'CBINFER_ROWCONV_MAXK': (16, "most output channels of a row-segment layer"),
    'CBINFER_NO_BLOCKCONV': (False, "no patch-staged block contraction (cb_blockconv.hip)"),
    'CBINFER_BLOCKCONV_MAXK': (64, "most output channels of a block-contraction layer"),
    'CBINFER_NO_ROWPAIRS': (False, "row-segment layers on cb_rowconv.hip instead of the row-pair kernel"),
    'CBINFER_NO_PAIRDET': (False, "a row-pair layer's change detection in a launch of its own"),
    'CBINFER_NO_NEXTFOLD': (False, "no consumer's change detection inside its producer's launch"),
    'CBINFER_NO_TAILFOLD': (False, "a fused 1x1 tail in a launch of its own"),
    'CBINFER_NO_WINFOLD': (False, "split-state producers stay in pixel order (no window-order fold)"),
    'CBINFER_NO_FASTPATH': (False, "no per-frame call plans: every frame takes the general path"),
    'CBINFER_NO_CHAINMASK': (False, "chained fp16 layers test every pixel, not only their producer's changed ones"),
    'CBINFER_NO_CHAIN': (False, "no chained frames (cbinfer_cbconv2d_forward_after); read at import"),
    'CBINFER_DIST_BACKEND': (None, "torch.distributed backend of shard.py (default: nccl on GPUs, else gloo)"),
    'CBINFER_FORCE_DIST': (False, "shard.py makes a process group also for one rank"),
}


# (os.environ's own table: os.environ.get raises and catches a KeyError for every unset name -- about 1.3 us against
#  0.1 us for this lookup -- and the split-state plans read six switches twice per layer and frame.  Do not go back to
#  os.environ.get here: it costs some 15 us per layer and frame.)
_ENVIRON, _ENV_KEYS = os.environ._data, {name: os.environ.encodekey(name) for name in SWITCHES}
_SPLIT_KEYS = tuple(_ENV_KEYS[name] for name in ('CBINFER_ARITH', 'CBINFER_EXACT_F32', 'CBINFER_NO_SPLIT',
                                                 'CBINFER_SPLIT_MINK', 'CBINFER_SPLIT_MAXK', 'CBINFER_NO_SELFCOMPACT'))


def _switch(name):
    default = SWITCHES[name][0]
    value = _ENVIRON.get(_ENV_KEYS[name])
    if value is None:
        return default
    value = os.environ.decodevalue(value)
    if default is True or default is False:
        return value == '1'
    return int(value) if type(default) is int else value


def _split_switches():
    """The raw values of the switches CBConv2d._split_ok reads: what a fast path that assumes its answer compares."""
    return tuple(map(_ENVIRON.get, _SPLIT_KEYS))


@contextlib.contextmanager
def _switch_set(name, value):
    """Set a switch for the duration of a with-block."""
    saved = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        os.environ.pop(name) if saved is None else os.environ.update({name: saved})


_NO_CHAIN = _switch('CBINFER_NO_CHAIN')


def _no_tag():
    return None


class _Produced(object):
    """What a CBConv2d leaves on its output buffer for the next layer (CBConv2d._note_upstream): who wrote it, in which
    of its frames, the buffer's version counter then, and where the frame's change count is.  Never travels: a pickled
    or deep-copied tensor carries None instead."""
    __slots__ = ('module', 'serial', 'version', 'count', 'tokens')

    def __init__(self, module, serial, version, count, tokens=()):
        self.module, self.serial, self.version, self.count = module, serial, version, count
        self.tokens = tokens      # (CBConv2d._half_detect_token of every consumer whose detection rode in the launch)

    def __reduce__(self):
        return _no_tag, ()

    def __deepcopy__(self, memo):
        return None


def _flush_side(pend):
    """The feedback refresh of a row-pair layer's state as a launch of its own (pend: frame, state, C, H, W, threshold)."""
    frame, state, Cn, H, W, th = pend
    check(C.cbinfer_refresh_state(ptr(frame), ptr(state), Cn, H, W, float(th), stream_ptr(frame)))


def _padding_pair(m, who):
    """The padding of the nn.Conv2d `m` as a pair of ints: ints as they are, 'valid', or a symmetric 'same'.
    CBinferError in the name of `who` otherwise."""
    Err = _lib.CBinferError
    k, d = tuple(m.kernel_size), tuple(m.dilation)
    if isinstance(m.padding, str):
        if m.padding == 'valid':
            return (0, 0)
        if m.padding == 'same':
            total = tuple(d[i] * (k[i] - 1) for i in (0, 1))
            if total[0] % 2 or total[1] % 2:
                raise Err("%s: padding='same' with kernel_size=%s, dilation=%s pads one side more than the "
                          "other (torch pads %s in total); only symmetric padding is supported" % (who, k, d, total))
            return (total[0] // 2, total[1] // 2)
        raise Err("%s: unknown padding %r" % (who, m.padding,))
    return tuple(int(v) for v in m.padding)


class CBConv2d(nn.Module):
    """Change-based 2-D convolution (reference: conv2d.py:87-304)."""

    def __init__(self, m, threshold, generalGeometry=False):
        super(CBConv2d, self).__init__()
        self.generalGeometry = bool(generalGeometry)
        if self.generalGeometry:
            padding = self._check_general(m)
        else:
            assert m.groups == 1 and m.transposed == False
            assert m.output_padding == (0, 0) and m.padding == (m.kernel_size[-2] // 2,
                                                                 m.kernel_size[-1] // 2)
            assert m.dilation == (1, 1) and m.stride == (1, 1)
            padding = m.padding
        self.groups = m.groups
        self.transposed = m.transposed
        self.output_padding = m.output_padding
        self.padding = padding
        self.dilation = m.dilation
        self.stride = m.stride
        self.kernel_size = m.kernel_size
        self.in_channels = m.in_channels
        self.out_channels = m.out_channels

        assert m.weight is not None and (m.bias is not None or self.generalGeometry)
        self.weight = m.weight   # shared with the source module, as in the reference
        self.bias = m.bias
        # a layer the unit-geometry kernels cannot take -- stride, dilation, free padding, an even filter size, no bias --
        # runs on cb_geomconv.hip (_path: 'geom'); any other layer built with generalGeometry=True runs as it always did
        kH, kW = self.kernel_size
        self._geom = self.generalGeometry and (
            tuple(self.stride) != (1, 1) or tuple(self.dilation) != (1, 1) or kH % 2 == 0 or kW % 2 == 0 or
            tuple(padding) != (kH // 2, kW // 2) or m.bias is None)
        self._geomC = None

        self.threshold = threshold
        self.clearMemory()

        self.withReLU = False
        self.saveChangeMap = False
        self.propChangeIndexes = False
        self.gatherComputationStats = False
        self.finegrained = False
        self.copyInput = True
        self.feedbackLoop = False
        # Extension: a layer fed propagated change indexes recomputes exactly the listed pixels (the reference's
        # behaviour, conv2d.py:180-190 -- short of the filter's reach for k > 1).  True: the list is first dilated by
        # the filter support on the device (cbinfer_dilate_change_indexes), as the layer's own detection would find.
        self.dilatePropagatedIndexes = False
        self._setDefaultValues()

    # ---------------------------------------------------------------- state
    def clearMemory(self):
        for name in ('prevInput', 'prevOutput'):
            if not hasattr(self, name):
                self.register_buffer(name, self.weight.detach().new_zeros(0))
            elif name not in self._buffers:
                tmp = getattr(self, name)
                delattr(self, name)
                self.register_buffer(name, tmp)
        self.prevInput = self.weight.detach().new_zeros(0)
        self.prevOutput = self.weight.detach().new_zeros(0)
        self.__dict__['_rangeFallback'] = False
        self.__dict__['_upSeen'] = None
        if hasattr(self, 'compStats'):
            self.compStats = None
        # device work buffers (not part of the module state)
        self._work = None
        self._plan = None
        self._lastIndexes = None

    def getStateTensors(self):
        return [getattr(self, n) for n in ('prevInput', 'prevOutput') if hasattr(self, n)]

    def _setDefaultValues(self):
        # back-fill attributes missing in modules pickled by older versions (conv2d.py:292-304)
        for name, val in (('saveChangeMap', False), ('propChangeIndexes', False), ('gatherComputationStats', False),
                          ('finegrained', False), ('copyInput', True), ('feedbackLoop', False), ('syncIndexes', False),
                          ('deterministicFG', False), ('atomicFG', False), ('fgInPlace', False), ('exactF32', False),
                          ('dilatePropagatedIndexes', False), ('_work', None), ('_wprep', None),
                          ('_inputIsLiveState', False), ('_plan', None), ('_wrows', None), ('_lastIndexes', None),
                          ('generalGeometry', False), ('_geom', False), ('_geomC', None)):
            if name not in self.__dict__:
                self.__dict__[name] = val

    def __getstate__(self):
        d = dict(self.__dict__)
        d.update(_work=None, _wprep=None, _plan=None, _wrows=None, _lastIndexes=None, _geomC=None)      # (transient device buffers)
        return d

    def __setstate__(self, state):
        super(CBConv2d, self).__setstate__(state)
        self._setDefaultValues()      # (a module pickled before an attribute existed loads with its default)

    def lastChangeIndexes(self):
        """The change list of the most recent coarse-grained frame as a ChangeIndexes (None before the first
        frame).  For mask-driven frames it is materialised on this call; valid until the next frame."""
        return self._lastIndexes

    def invalidateWeights(self):
        """Forget the cached re-laid-out copies of the filter bank and the call plan -- after a write through
        `weight.data`, which bumps neither the Parameter object nor its version counter."""
        self._wprep = self._wrows = self._plan = None

    # ---------------------------------------------------------------- general geometry (cb_geomconv.hip)
    @staticmethod
    def _check_general(m):
        """The padding of `m` as a pair of ints if CBConv2d(m, th, generalGeometry=True) takes the module: any stride,
        dilation and zero padding within the library's limits, with or without bias.  CBinferError otherwise."""
        Err = _lib.CBinferError
        if not isinstance(m, nn.Conv2d) or m.transposed or tuple(m.output_padding) != (0, 0):
            raise Err("CBConv2d: only plain nn.Conv2d modules are converted (no transposed convolution)")
        if m.groups != 1:
            raise Err("CBConv2d: grouped and depthwise convolutions are not supported (groups=%d)" % m.groups)
        if m.padding_mode != 'zeros':
            raise Err("CBConv2d: padding_mode=%r is not supported, only 'zeros'" % (m.padding_mode,))
        k, d = tuple(m.kernel_size), tuple(m.dilation)
        padding = _padding_pair(m, 'CBConv2d')
        g = _lib.Geom(k[0], k[1], m.stride[0], m.stride[1], padding[0], padding[1], d[0], d[1])
        if C.cbinfer_geom_prepared_weights_bytes(m.out_channels, m.in_channels, ctypes.byref(g), _lib.CB_F32) <= 0:
            raise Err("CBConv2d: kernel_size=%s stride=%s padding=%s dilation=%s is beyond what the library takes "
                      "(per axis: filter <= 7, stride <= 4, dilation <= 8, padding <= 64)"
                      % (k, tuple(m.stride), padding, d))
        return padding

    def _geom_struct(self):
        """(pointer to) the layer's cbGeom; transient, made again after unpickling."""
        if self.__dict__.get('_geomC') is None:
            k, s_, p_, d = self.kernel_size, self.stride, self.padding, self.dilation
            self.__dict__['_geomC'] = ctypes.pointer(_lib.Geom(k[0], k[1], s_[0], s_[1], p_[0], p_[1], d[0], d[1]))
        return self.__dict__['_geomC']

    def _out_hw(self, Hi, Wi):
        """Output map of an Hi x Wi input map (torch's formula; the input map itself for a unit-geometry layer)."""
        if not self.__dict__.get('_geom'):
            return Hi, Wi
        Ho, Wo = ctypes.c_int(), ctypes.c_int()
        if C.cbinfer_geom_out_size(Hi, Wi, self._geom_struct(), ctypes.byref(Ho), ctypes.byref(Wo)) != 0:
            raise _lib.CBinferError("CBConv2d: a %dx%d map is smaller than the filter's reach (kernel_size=%s, dilation=%s, "
                                    "padding=%s)" % (Hi, Wi, tuple(self.kernel_size), tuple(self.dilation),
                                                     tuple(self.padding)))
        return Ho.value, Wo.value

    def _geom_workspace(self, input, Ho, Wo):
        key = (input.size(-2), input.size(-1), input.device, 'geom')
        if self._work is None or self._work['key'] != key:
            dev = input.device
            self._work = dict(
                key=key, selfc=True,
                bits=torch.zeros(C.cbinfer_frame_mask_bytes(Ho, Wo) // 8, dtype=torch.int64, device=dev),
                idx=torch.empty(Ho * Wo, dtype=torch.int32, device=dev),
                count=torch.zeros(1, dtype=torch.int32, device=dev),
                conv=torch.zeros(C.cbinfer_geom_workspace_bytes(), dtype=torch.uint8, device=dev),
                map=None, rows=None, split=None)
        return self._work

    def _geom_weights(self, Hi, Wi, arith):
        w = self.weight
        key = ('geom', w.data_ptr(), w._version, w.dtype, w.device, Hi, Wi, arith)
        if self._wprep is None or self._wprep[0] != key:
            K, Cin = w.size(0), w.size(1)
            g = self._geom_struct()
            wp = torch.empty(C.cbinfer_geom_prepared_weights_bytes(K, Cin, g, arith), dtype=torch.uint8, device=w.device)
            check(C.cbinfer_geom_prep_weights(ptr(w.detach().contiguous()), ptr(wp), K, Cin, Hi, Wi, g, arith,
                                              stream_ptr(w)))
            self._wprep = (key, wp)
        return self._wprep[1]

    def _forward_geom(self, inp):
        """A frame of a general-geometry layer: cbinfer_cbconv2d_forward_geom, two launches, no host sync.  Change list,
        prevOutput and the indexes handed on live on the OUTPUT map."""
        Err = _lib.CBinferError
        changeIndexes = None
        if isinstance(inp, LazyPool):      # (_path(pooled=True) == 'dense')
            inp = inp.tensor()
        src = inp[1] if type(inp) == tuple else inp
        self._inputIsLiveState = bool(getattr(src, '_cbinfer_inplace_state', False))
        input = src.detach().contiguous()
        assert input.dim() == 4 and input.size(0) == 1 and input.size(-3) == self.in_channels
        require_device(input)
        assert input.dtype == self.weight.dtype, "input and weights must have the same dtype"
        K, Cin = self.weight.size(0), self.weight.size(1)
        Hi, Wi = input.size(-2), input.size(-1)
        Ho, Wo = self._out_hw(Hi, Wi)
        have = type(inp) == tuple
        if have:
            assert inp[0] == 'changeIndexes'
            changeIndexes = inp[2]
            if (Ho, Wo) != (Hi, Wi):
                raise Err("CBConv2d: propagated change indexes address this layer's %dx%d INPUT map, its change list lives "
                          "on the %dx%d output map (kernel_size=%s stride=%s padding=%s dilation=%s): such a layer runs "
                          "its own change detection" % (Hi, Wi, Ho, Wo, tuple(self.kernel_size), tuple(self.stride),
                                                        tuple(self.padding), tuple(self.dilation)))
            if self.feedbackLoop:
                raise Err("CBConv2d: feedbackLoop=True cannot be combined with propagated change indexes (the layer "
                          "state would never be updated)")
            if isinstance(changeIndexes, ChangeIndexes):
                if changeIndexes.size not in (None, (Hi, Wi)):
                    raise Err("CBConv2d: the propagated change indexes address a %dx%d map, this layer runs at %dx%d"
                              % (changeIndexes.size + (Hi, Wi)))
                idx, count = changeIndexes.buffer, changeIndexes.count
            else:
                idx = changeIndexes.detach().contiguous()
                count = torch.full((1,), idx.numel(), dtype=torch.int32, device=input.device)
            if idx.dtype != torch.int32 or not idx.is_contiguous():
                raise Err("CBConv2d: propagated change indexes must be a contiguous int32 tensor")
            cap = min(idx.numel(), Ho * Wo)
        self._state_for(input.size(), input)
        if self.gatherComputationStats:
            self._gatherStats(input)
        work = self._geom_workspace(input, Ho, Wo)
        if not have:
            idx, count, cap = work['idx'], work['count'], Ho * Wo
        if not self.prevInput.is_contiguous():
            self.prevInput = self.prevInput.contiguous()
        arith = self._arith(input)
        bias = self.bias.detach() if self.bias is not None else None
        args = (ptr(input), ptr(self.prevInput), ptr(self.prevOutput), ptr(work['bits']), ptr(idx), ptr(count),
                ptr(self._geom_weights(Hi, Wi, arith)), ptr(bias), Cin, Hi, Wi, K, self._geom_struct(),
                float(self.threshold), int(bool(self.feedbackLoop)), int(bool(self.copyInput)), int(bool(self.withReLU)),
                int(have), cap, ptr(work['conv']), arith, stream_ptr(input))
        check(C.cbinfer_cbconv2d_forward_geom(*args))
        result = changeIndexes if have else ChangeIndexes(idx, count, (Ho, Wo))
        if self.saveChangeMap and not have:
            # the frame's mask, left behind the two alternating ones, expanded to an int8 [Ho, Wo] map (list and count
            # are written again with what they hold)
            if work['map'] is None:
                work['map'] = torch.zeros(Ho, Wo, dtype=torch.int8, device=input.device)
            off = C.cbinfer_frame_mask_copy_offset(Ho, Wo) // 8
            check(C.cbinfer_compact_bits(ptr(work['bits'][off:]), Wo, Ho, ptr(idx), ptr(count), None, ptr(work['map']),
                                         stream_ptr(input)))
            self.changeMap = work['map']
        if not self.feedbackLoop and not self.copyInput:
            self.prevInput = input.clone() if self._inputIsLiveState else input
        elif not have and not self._inputIsLiveState:
            self._make_plan(False, input, C.cbinfer_cbconv2d_forward_geom, args, 0)
            if self._plan is not None:
                self._plan['indexes'] = result
        return self._emit(result)

    def _rows_path(self, dtype, H, W):
        """Which mask-driven contraction, if any, runs this layer's sync-free fp32 frame (no int8 mask copy): 'rows'
        (cb_rowconv.hip, at most 16 output channels), 'blocks' (cb_blockconv.hip, bf16x3 arithmetic, 17..64 output
        channels) or None: the list kernel (cb_conv.hip), whose 64-pixel tiles reuse the weights better beyond."""
        K, Cin, kH, kW = self.weight.size()
        if dtype != torch.float32 or self.syncIndexes or self.saveChangeMap or _switch('CBINFER_NO_SELFCOMPACT'):
            return None
        if (K <= _switch('CBINFER_ROWCONV_MAXK') and not _switch('CBINFER_NO_ROWCONV') and
                C.cbinfer_rowconv_supported(Cin, K, kH, kW)):
            return 'rows'
        if (K <= _switch('CBINFER_BLOCKCONV_MAXK') and self._arith_code(dtype) == _lib.CB_F32S and
                not _switch('CBINFER_NO_BLOCKCONV') and C.cbinfer_blockconv_supported(Cin, K, kH, kW)):
            return 'blocks'
        return None

    def _relaid(self, key, nbytes, prep, extra=lambda w: ()):
        """(buffer, *extra(weights)): the filter bank re-laid out for one kernel family by prep(weights, buffer, K, Cin,
        kH, kW, *extra(weights), stream) into nbytes(Cin, K, kH, kW) bytes.  One such copy at a time, made again when the
        weights or `key` change; `extra` is evaluated only then."""
        w = self.weight
        key = key + (w.data_ptr(), w._version, w.device)
        if self._wrows is None or self._wrows[0] != key:
            K, Cin, kH, kW = w.size()
            more = tuple(extra(w))
            wp = torch.empty(nbytes(Cin, K, kH, kW), dtype=torch.uint8, device=w.device)
            check(prep(ptr(w.detach().contiguous()), ptr(wp), K, Cin, kH, kW, *more, stream_ptr(w)))
            self._wrows = (key, wp) + more
        return self._wrows[1:]

    def _masked_call(self, path):
        """(library entry point, prepared weights) of a mask-driven path."""
        if path == 'rows':
            return C.cbinfer_cbconv2d_forward_rows, self._relaid(
                ('rows',), C.cbinfer_rowconv_prepared_bytes, C.cbinfer_rowconv_prep_weights)[0]
        return C.cbinfer_cbconv2d_forward_blocks, self._relaid(
            ('blocks',), C.cbinfer_blockconv_prepared_bytes, C.cbinfer_blockconv_prep_weights)[0]

    def _pairs_ok(self, H, W):
        """Does the row-segment frame of this layer run on the row-PAIR kernel (cb_rowpair.hip: persistent over the
        non-empty (row pair, mask word) units, and able to do the next layer's pooled detection)?  Feedback mode, at
        most 4 input and 16 output channels, 3x3 / 5x5 / 7x7; CBINFER_NO_ROWPAIRS=1 switches it off."""
        K, Cin, kH, kW = self.weight.size()
        return (self.feedbackLoop and not _switch('CBINFER_NO_ROWPAIRS') and
                bool(C.cbinfer_rowpairs_supported(Cin, K, kH, kW, H, W)))

    def _pair_detect_ok(self, nxt, kH):
        """Does this row-pair layer run its own change detection inside its launch (cbinfer_conv_rowpairs_detect)?  Only
        while the consumer behind the pool takes its detection from this launch (nxt) and its last frame ran a contraction
        that can carry this layer's state refresh on idle workgroups (cbinfer_split_conv_[next_]refresh)."""
        if nxt is None or kH != 7 or _switch('CBINFER_NO_PAIRDET'):
            return False
        link = self.__dict__.get('_fusedNext')
        cons = link[1] if link is not None else None
        cp = cons.__dict__.get('_plan') if cons is not None else None
        return bool(cp is not None and cp.get('split') and cp.get('sideArgs') is not None)

    def _detect_token(self):
        """What a producer that ran this layer's pooled detection inside its own launch must have seen: the identity of
        the state buffers and the threshold.  None while this layer cannot take such a detection (no split-state frame
        yet, a state that was written from outside and must be re-split, a threshold that differs from last frame's)."""
        sp = self._work.get('split') if self._work else None
        prev = self._buffers['prevInput']
        if (sp is None or sp['stateKey'] != (prev.data_ptr(), prev._version) or self.__dict__.get('_rangeFallback') or
                self.__dict__.get('_pmaskThreshold') != float(self.threshold)):
            return None
        return self._split_token(sp, prev)

    def _split_token(self, sp, prev):
        """The detection token of this layer's split-state frame (state buffers, threshold, arithmetic)."""
        return (id(self), prev.data_ptr(), sp['S'].data_ptr(), sp['bits'].data_ptr(), float(self.threshold),
                sp['arith'])

    def _next_detect(self, H, W):
        """(cbNextDetect, token) if this layer's row-pair launch can also be the pooled change detection of the layer
        behind the following CBPoolMax2d (pycbinfer.fuseDetectionIntoProducer), else (None, None)."""
        link = self.__dict__.get('_fusedNext')
        if link is None or self.__dict__.get('_noNextFold') or _switch('CBINFER_NO_NEXTFOLD'):
            return None, None
        pool, cons = link
        if type(cons) is not CBConv2d or cons.__dict__.get('_geom') or self.__dict__.get('_geom'):
            return None, None      # (a general-geometry layer folds no detection and has none folded)
        # (runs every frame inside the call plans: the outcome is reused while every input of the test below is what it
        #  was -- the consumer's state and threshold by its token, everything else, both sides, by `key`)
        w, w2, prev2 = self._parameters['weight'], cons._parameters['weight'], cons._buffers.get('prevInput')
        key = (getattr(pool, 'lazy', False), pool.propChangeIndexes, pool.ceil_mode, cons.feedbackLoop, cons.copyInput,
               cons.syncIndexes, cons.saveChangeMap, cons.gatherComputationStats, cons.finegrained, cons.exactF32,
               w2.dtype, w2.shape, None if prev2 is None else (prev2.shape, prev2.device), H, W, _split_switches(),
               w.shape[0], w.device)
        tok = cons._detect_token()
        nd = self.__dict__.get('_nextStruct')
        if nd is not None and nd[0] == tok and nd[2] == key:
            return nd[1], tok
        K = w.size(0)
        if (not key[0] or pool.propChangeIndexes or cons.in_channels != K or not cons.feedbackLoop or cons.syncIndexes or
                cons.saveChangeMap or cons.gatherComputationStats or cons.finegrained or w2.dtype != torch.float32):
            return None, None
        H2, W2 = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if pool.ceil_mode else (H // 2, W // 2)
        if (prev2 is None or tuple(prev2.shape) != (1, K, H2, W2) or prev2.device != w.device or
                not cons._split_ok(torch.float32, H2, W2) or tok is None):
            return None, None
        if nd is None or nd[0] != tok:
            sp = cons._work['split']
            st = _lib.NextDetect()
            st.state, st.splitState, st.frameMasks = prev2.data_ptr(), sp['S'].data_ptr(), sp['bits'].data_ptr()
            st.rangeFlag, st.H, st.W = sp['flag'].data_ptr(), H2, W2
            st.kH, st.kW, st.threshold = w2.size(2), w2.size(3), float(cons.threshold)
            st.arith = 1 if sp['arith'] == 'x3' else 0
            nd = (tok, st)
        self.__dict__['_nextStruct'] = (tok, nd[1], key)
        return nd[1], tok

    def _rows_workspace(self, work, H, W, dev):
        if work['rows'] is None:
            words = C.cbinfer_mask_words(H, W)
            work['rows'] = dict(bits=torch.zeros(words, dtype=torch.int64, device=dev),
                                arrive=torch.zeros(words, dtype=torch.int32, device=dev),
                                copy=torch.zeros(words, dtype=torch.int64, device=dev))
        return work['rows']

    @staticmethod
    def _split_arith():
        """Arithmetic of the split-state kernels for fp32 layers (CBINFER_ARITH): 'x3' (default: bf16 triples, every f32
        operand exactly, f32-equivalent) or 'f16x2' (f16 pairs, 22-23 significant bits per operand); None for any
        other value ('bf16x3'), which keeps the layer on the list / patch-staged kernels."""
        a = _switch('CBINFER_ARITH')
        return a if a in ('x3', 'f16x2') else None

    def _arith_code(self, dtype):
        if dtype == torch.float16:
            return _lib.CB_F16
        if not self.exactF32 and not _switch('CBINFER_EXACT_F32'):
            return _lib.CB_F32S
        return _lib.CB_F32

    def _arith(self, t):
        """Arithmetic code of the list / patch-staged kernels: fp16 as is; fp32 as split bf16x3 products on the 16-bit
        MFMA (CB_F32S, which also admits the split-state kernels) unless exactF32 asks for the f32 MFMA (CB_F32)."""
        dtype_code(t)     # (rejects anything but fp32 / fp16)
        return self._arith_code(t.dtype)

    def _prepared_weights(self, H=1, W=1, arith=None):
        w = self.weight
        key = (w.data_ptr(), w._version, w.dtype, w.device, H, W, arith)
        if self._wprep is None or self._wprep[0] != key:
            self._wprep = (key, prepWeights(w, H, W, arith=arith))
        return self._wprep[1]

    # ---------------------------------------------------------------- split-state frame (cb_split.hip)
    def _split_ok(self, dtype, H, W):
        """Does this layer's sync-free frame run on the split-state kernels (cbinfer_split_forward)?  fp32 in the split
        products' arithmetic, a layer that keeps its input (feedback or copy), a shape the library takes."""
        K = self.weight.size(0)
        return ((self.feedbackLoop or self.copyInput) and not self.syncIndexes and not self.saveChangeMap
                and not self.finegrained and self._split_kernels_ok(dtype, H, W)
                and _switch('CBINFER_SPLIT_MINK') <= K <= _switch('CBINFER_SPLIT_MAXK')
                and not _switch('CBINFER_NO_SELFCOMPACT'))

    def _split_kernels_ok(self, dtype, H, W):
        """What both split-state frames need: fp32 in the split products' arithmetic, the library takes the shape."""
        K, Cin, kH, kW = self.weight.size()
        return (dtype == torch.float32 and self._arith_code(dtype) == _lib.CB_F32S
                and (not self.__dict__.get('_rangeFallback') or self._split_arith() == 'x3')
                and not _switch('CBINFER_NO_SPLIT') and self._split_arith() is not None
                and _split_fits(Cin, K, kH, kW, H, W))

    def _hsplit_ok(self, dtype, H, W):
        """Does this fp16 layer's sync-free frame run on the split-state machinery (cbinfer_hsplit_forward: pixel-major
        f16 copy of the state, LDS-DMA contraction)?  Input channels a multiple of 64, feedback mode or a layer that
        keeps a copy of its input; CBINFER_NO_HSPLIT=1 (or CBINFER_NO_SPLIT=1) switches it off."""
        K, Cin, kH, kW = self.weight.size()
        return (dtype == torch.float16 and (self.feedbackLoop or self.copyInput)
                and not self.syncIndexes and not self.saveChangeMap and not self.finegrained
                and not _switch('CBINFER_NO_SPLIT') and not _switch('CBINFER_NO_HSPLIT')
                and not _switch('CBINFER_NO_SELFCOMPACT')
                and bool(C.cbinfer_hsplit_supported(Cin, K, kH, kW))
                # (deep contractions, 48 k-stages and more, unless CBINFER_HSPLIT_DEEP=0; channels padded to a multiple
                #  of 64 -- OpenPose's 185 -> 192 -- by up to a quarter)
                and (kH * kW * ((Cin + 63) // 64) < 48 or _switch('CBINFER_HSPLIT_DEEP'))
                and 4 * ((Cin + 63) // 64 * 64 - Cin) <= (Cin + 63) // 64 * 64
                and C.cbinfer_mask_words(H, W) <= C.cbinfer_hsplit_max_mask_words(K)
                and C.cbinfer_hsplit_state_bytes(Cin, H, W, kH, kW) < (1 << 31) and H * W * W < (1 << 32))

    def _forward_hsplit(self, input, work, lazy=None):
        """One fp16 frame on the split-state machinery: detection + refresh of the state and its pixel-major copy, then
        the contraction, whose launch may also run its consumers' detection (and whose own detection is skipped when its
        producer's launch did it).  `lazy`: behind a folded CBPoolMax2d, `input` is the pool's input."""
        K, Cin, kH, kW = self.weight.size()
        H, W = (lazy.outSize[-2], lazy.outSize[-1]) if lazy is not None else (input.size(-2), input.size(-1))
        dev = input.device
        hs = work.get('hsplit')
        if hs is None:
            S = torch.empty(C.cbinfer_hsplit_state_bytes(Cin, H, W, kH, kW), dtype=torch.uint8, device=dev)
            check(C.cbinfer_hsplit_state_init(ptr(S), Cin, H, W, kH, kW, stream_ptr(S)))
            wsBytes = C.cbinfer_hsplit_workspace_bytes(Cin, H, W, K, kH, kW)
            hs = work['hsplit'] = dict(
                S=S, bits=torch.zeros(C.cbinfer_frame_mask_bytes(H, W) // 8, dtype=torch.int64, device=dev),
                copy=torch.zeros(C.cbinfer_mask_words(H, W), dtype=torch.int64, device=dev),
                ws=torch.zeros(wsBytes, dtype=torch.uint8, device=dev) if wsBytes > 0 else None, stateKey=None,
                layer=(_lib.HalfLayer * 1)())
        wp = self._relaid(('hsplit', H, W), C.cbinfer_hsplit_prepared_bytes, C.cbinfer_hsplit_prep_weights,
                          lambda w: (H, W))[0]
        prev = self.prevInput
        if not prev.is_contiguous():
            prev = self.prevInput = prev.contiguous()
        stateKey = (prev.data_ptr(), prev._version)
        rebuilt = hs['stateKey'] != stateKey
        if rebuilt:
            # first frame on this path, or prevInput was (re)allocated or written by somebody else: the pixel-major
            # copy is made again from it
            check(C.cbinfer_hsplit_state_rebuild(ptr(prev), ptr(hs['S']), Cin, H, W, kH, kW, stream_ptr(input)))
            hs['stateKey'] = stateKey
        pooled = lazy is not None
        ok = self._pmask_ok(rebuilt)
        # (round 5: a chained layer skips the segments its producer left alone)
        pmask = (lazy.producerMask() if pooled else self._chain_mask(H, W)) if ok else None
        L = hs['layer'][0]
        L.upstreamCount, L.input, L.producerMask = None, ptr(input), ptr(pmask)
        L.state, L.pixelState, L.frameMasks = ptr(prev), ptr(hs['S']), ptr(hs['bits'])
        L.output, L.idxOut, L.countOut = ptr(self.prevOutput), ptr(work['idx']), ptr(work['count'])
        L.maskCopy, L.prepared, L.bias = ptr(hs['copy']), ptr(wp), ptr(self.bias.detach())
        L.K, L.threshold, L.relu = K, float(self.threshold), int(bool(self.withReLU))
        # this layer's own detection: done by the producing layer's launch?  (never on a fresh / restored state, after a
        # change of the threshold, or behind a pool)
        mine = self._half_token(hs, prev) if (ok and not pooled) else None
        L.detect = 0 if (mine is not None and self._detected_upstream(mine)) else 1
        tokens = self._fill_consumers(L, H, W)
        args = [hs['layer'], 1, int(pooled), input.size(-2) if pooled else 0, input.size(-1) if pooled else 0,
                Cin, H, W, kH, kW, int(bool(self.feedbackLoop)), ptr(hs['ws']), stream_ptr(input)]
        check(C.cbinfer_hsplit_forward_group(*args))
        self.__dict__['_ranSplit'] = True      # (a frame on any OTHER path invalidates hs['stateKey'], see forward)
        self._publish_count(work['count'], tokens)
        if not self._inputIsLiveState:
            self._make_plan(pooled, input, C.cbinfer_hsplit_forward_group, args, None, pmask=ptr(pmask))
            if self._plan is not None:
                self._plan.update(hsplit=True, chain=True, stateVersion=prev._version, checkPmask=pooled,
                                  layer=L, size=(H, W), hs=hs)
        self._lastIndexes = MaskChangeIndexes(hs['copy'], (H, W), work['idx'], work['count'], made=True)
        if self._plan is not None:
            self._plan['indexes'] = self._lastIndexes
        return self._emit(self._lastIndexes)

    # ---- the change detection of an fp16 layer inside the launch of the layer that PRODUCES its input ----
    # A consumer in copy mode compares the producer's output buffer with a copy of last frame's, so only the pixels the
    # producer just recomputed can trigger, and the producer's launch can do the whole detection for them.  Checked on
    # the host every frame from both sides, with a token naming the consumer's state buffers and threshold: the PRODUCER
    # folds a consumer in only if that consumer's last frame consumed this producer's last frame from this very buffer
    # (its _upSeen); the CONSUMER skips its detection only if the tag on its input carries its token of this frame.
    def _half_token(self, hs, prev):
        return (id(self), prev.data_ptr(), hs['S'].data_ptr(), hs['bits'].data_ptr(), float(self.threshold))

    def _detected_upstream(self, token):
        d = self.__dict__
        return (d.get('_upNow') is not None and token in (d.get('_upTokens') or ()) and
                not _switch('CBINFER_NO_NEXTFOLD'))

    def _half_detect_token(self, prod, prodSerial, pout, H, W):
        """The token under which `prod`'s launch of its NEXT frame may run this layer's change detection, or None."""
        d = self.__dict__
        if (self.feedbackLoop or not self.copyInput or self.syncIndexes or self.saveChangeMap or
                self.gatherComputationStats or self.finegrained or not d.get('_ranSplit')):
            return None
        work = self._work
        hs = work.get('hsplit') if work else None
        prev = self._buffers.get('prevInput')
        if (hs is None or prev is None or prev.dtype != torch.float16 or
                tuple(prev.shape) != (1, prod.out_channels, H, W) or
                hs['stateKey'] != (prev.data_ptr(), prev._version)):
            return None
        seen = d.get('_upSeen')
        if (seen is None or seen[0] is not prod or seen[1] != prodSerial or seen[2] != pout.data_ptr() or
                seen[3] != prev.data_ptr() or seen[4] != prev._version):
            return None
        if d.get('_pmaskThreshold') != float(self.threshold):
            return None
        return self._half_token(hs, prev)

    def _fill_consumers(self, L, H, W):
        """cbHalfLayer.next[] of this frame: the linked consumers (pycbinfer.fuseDetectionIntoProducer) whose detection
        this launch may run.  Returns their tokens."""
        L.nNext = 0
        links = self.__dict__.get('_fusedConsumers')
        if not links or _switch('CBINFER_NO_NEXTFOLD') or self.weight.size(0) < 64:
            return ()
        pout = self._buffers['prevOutput']
        tag = getattr(pout, '_cbProduced', None)      # (still the PREVIOUS frame's)
        serial = self.__dict__.get('_serial', 0)
        if tag is None or tag.module is not self or tag.serial != serial - 1 or pout._version != tag.version:
            return ()
        tokens = []
        for cons in links:
            if len(tokens) == _lib.HNEXT_MAX:
                break
            tok = cons._half_detect_token(self, serial - 1, pout, H, W) if type(cons) is CBConv2d else None
            if tok is None:
                continue
            n = L.next[len(tokens)]
            n.state, n.pixelState, n.frameMasks = tok[1], tok[2], tok[3]
            n.kH, n.kW, n.threshold = cons.weight.size(2), cons.weight.size(3), tok[4]
            tokens.append(tok)
        L.nNext = len(tokens)
        return tuple(tokens)

    def _split_fg_ok(self, dtype, H, W):
        """Does this layer's fine-grained in-place frame run on the split-state kernels (cbinfer_split_forward_fg)?
        As _split_ok, for a layer in fine-grained mode."""
        return not _switch('CBINFER_NO_SPLIT_FG') and self._split_kernels_ok(dtype, H, W)

    def _split_weights(self, H, W):
        """(prepared buffer, weight scale).  f16 pairs: a power of two with max |w| * scale in [2^13, 2^14); bf16
        triples ('x3'): the weights as they are -- scale 0.0, which is also what tells the library's frame functions
        which form the buffers hold (include/cbinfer_hip.h)."""
        if self._split_arith() == 'x3':
            return self._relaid(('x3', H, W), C.cbinfer_split3_prepared_bytes, C.cbinfer_split3_prep_weights,
                                lambda w: (H, W))[0], 0.0

        def scaled(w):
            wmax = float(w.detach().abs().max())          # (one host sync when the weights change)
            return H, W, 2.0 ** (13 - math.floor(math.log2(wmax))) if wmax > 0 and math.isfinite(wmax) else 1.0
        wp, _, _, scale = self._relaid(('f16x2', H, W), C.cbinfer_split_prepared_bytes, C.cbinfer_split_prep_weights,
                                       scaled)
        return wp, scale

    def _split_workspace(self, work, H, W, dev):
        sp = work.get('split')
        arith = self._split_arith()
        if sp is None or sp['arith'] != arith:      # (the records of the two arithmetics differ in size and content)
            K, Cin, kH, kW = self.weight.size()
            words = C.cbinfer_mask_words(H, W)
            x3 = arith == 'x3'
            S = torch.empty((C.cbinfer_split3_state_bytes if x3 else C.cbinfer_split_state_bytes)(Cin, H, W, kH, kW),
                            dtype=torch.uint8, device=dev)
            check((C.cbinfer_split3_state_init if x3 else C.cbinfer_split_state_init)(ptr(S), Cin, H, W, kH, kW,
                                                                                      stream_ptr(S)))
            # (slabs only for deep contractions -- 48 k-stages and more: 0 bytes otherwise)
            wsBytes = C.cbinfer_split_workspace_bytes(1, Cin, H, W, K, kH, kW)
            ws = torch.zeros(wsBytes, dtype=torch.uint8, device=dev) if wsBytes > 0 else None
            # (a frame mask of its own: the list and split-state kernels' mask protocols must never share a buffer)
            sp = work['split'] = dict(S=S, arith=arith, flag=torch.zeros(1, dtype=torch.int32, device=dev),
                                      bits=torch.zeros(C.cbinfer_frame_mask_bytes(H, W) // 8, dtype=torch.int64,
                                                       device=dev),
                                      copy=torch.zeros(words, dtype=torch.int64, device=dev), ws=ws,
                                      stateKey=None, seq=(_lib.SplitSeq * 1)())
        return sp

    def _fill_seq(self, sp, work, src, pmask):
        """The split-state record (cbSplitSeq) of this frame's buffers."""
        q = sp['seq'][0]
        q.input, q.state, q.splitState = src.data_ptr(), self.prevInput.data_ptr(), sp['S'].data_ptr()
        q.frameMasks, q.producerMask = sp['bits'].data_ptr(), ptr(pmask)
        q.output, q.idxOut, q.countOut = self.prevOutput.data_ptr(), work['idx'].data_ptr(), work['count'].data_ptr()
        q.rangeFlag, q.maskCopy = sp['flag'].data_ptr(), sp['copy'].data_ptr()
        return q

    def _folded_tail(self, sp, H, W, dev):
        """The CBTail1x1 behind this layer if its evaluation can ride in this layer's second launch
        (cbinfer_split_forward_tail), with sp['tail'] (cbSplitTail) filled in -- else None (it runs its own launch)."""
        t = self._fusedTailCandidate()
        K, Cin, kH, kW = self.weight.size()
        if (t is None or sp['ws'] is None or t.in_channels != K or
                t.weight1.dtype != torch.float32 or t.weight1.device != dev or
                # (the second launch reads the layer's bias and the tail's first four values at a time)
                (self.bias.data_ptr() | t.bias1.data_ptr()) & 15 or
                not C.cbinfer_split_tail_supported(Cin, K, kH, kW, t.hidden_channels, t.out_channels)):
            return None
        out = t._output_for(H, W, dev, torch.float32)
        st = sp.get('tail')
        if st is None:
            st = sp['tail'] = _lib.SplitTail()
        sp['tailKeep'] = (t._prepared(), t.bias1.detach(), t.weight2.detach().contiguous(), t.bias2.detach())
        st.w1Prepared, st.b1, st.w2, st.b2 = [x.data_ptr() for x in sp['tailKeep']]
        st.C1, st.C2, st.relu1, st.relu2 = t.hidden_channels, t.out_channels, int(t.relu), int(bool(t.withReLU))
        st.output[0] = out.data_ptr()
        return t

    def _fusedTailCandidate(self):
        """The fused tail this layer would fold into its second launch right now (_folded_tail's cheap part), or None."""
        t = self.__dict__.get('_fusedTail')
        if t is None or not self.propChangeIndexes or self.__dict__.get('_noTailFold') or _switch('CBINFER_NO_TAILFOLD'):
            return None
        return t

    def _tail_unchanged(self, plan):
        """Does a split-state plan's tail folding still hold (a FramePipeline may take it away or give it back)?"""
        t = plan['tail']
        return self._fusedTailCandidate() is plan['tailCand'] and (t is None or t._fold_key() == plan['tailKey'])

    def rangeExceeded(self):
        """True if a state value of this layer ever left the range of the f16-pair arithmetic (|x| >= 2^20, or a
        non-finite input) since the state was cleared (one host sync unless the module has noticed already).  The
        outputs are right either way: the kernel computes such frames in plain f32 (cbs_exact_tile), slowly, until
        `_poll_range` moves the layer to the bf16x3 kernels."""
        if self.__dict__.get('_rangeFallback'):
            return True
        sp = self._work.get('split') if self._work else None
        return bool(sp is not None and int(sp['flag'].item()) != 0)

    def _poll_range(self, sp):
        """Every 64th split-state frame: an asynchronous copy of the range flag into pinned memory and a look at what the
        previous copy brought (no sync).  A tripped flag moves the layer to the bf16x3 kernels until clearMemory."""
        if sp['arith'] == 'x3':      # (bf16 triples have f32's range: the flag is never set)
            return
        n = sp['poll'] = sp.get('poll', 0) + 1
        if n & 63 or torch.cuda.is_current_stream_capturing():
            return
        host, ev = sp.get('flagHost'), sp.get('flagEvent')
        if host is None:
            host = sp['flagHost'] = torch.zeros(1, dtype=torch.int32).pin_memory()
        elif ev is not None and ev.query() and int(host[0]) != 0:
            self.__dict__['_rangeFallback'] = True
            self._plan = None
            return
        host.copy_(sp['flag'], non_blocking=True)
        ev = sp['flagEvent'] = torch.cuda.Event()
        ev.record()

    def _window_fold(self, sp, tail, H, W):
        """Can this split-state layer's contraction run in pooling-window order and carry the pooled change detection of
        the layer behind the following CBPoolMax2d (cbinfer_split_*_next)?  -> (eligible at all, cbNextDetect or None, the
        token the consumer will look for or None, _next_detect's token before the library's own test).  windowOrder of
        pycbinfer.fuseDetectionIntoProducer: True, False or 'auto' (DESIGN 5.8); CBINFER_NO_WINFOLD=1 switches it off."""
        K, Cin, kH, kW = self.weight.size()
        mode = self.__dict__.get('_winFold', 'auto')
        eligible = tail is None and sp['arith'] == 'x3' and mode is not False and not _switch('CBINFER_NO_WINFOLD')
        nxt, ntok, rawTok = None, None, None
        if eligible:
            nxt, ntok = self._next_detect(H, W)
            rawTok = ntok
            if nxt is not None and not C.cbinfer_split_next_supported(Cin, K, kH, kW, H, W, ctypes.pointer(nxt)):
                nxt, ntok = None, None
            if nxt is not None and mode == 'auto':
                # decided ONCE per module, when a call plan is made outside any capture, from the first frame that
                # recomputed some but not all pixels: the form pays while its tiles of 16 windows (+ ~20 % for a touched
                # window's unchanged pixels) fit one round of the persistent grid.  Until then (four looks): used.
                st = self.__dict__.setdefault('_winAuto', {'fold': None, 'looks': 0})
                if st['fold'] is None and not torch.cuda.is_current_stream_capturing():
                    n = int(self._work['count'].item())
                    st['looks'] += 1
                    if 0 < n < H * W:
                        cus = torch.cuda.get_device_properties(self.weight.device).multi_processor_count
                        st['fold'] = (1.2 * n) / 64.0 <= cus
                    elif st['looks'] >= 4:
                        st['fold'] = True
                if st['fold'] is False:
                    nxt, ntok = None, None
        return eligible, nxt, ntok, rawTok

    def _forward_split(self, src, lazy, work):
        """One frame on the split-state kernels: detection (+ pooling) + refresh of prevInput and of its pre-split
        copy, then the LDS-DMA contraction.  `src` is the layer input, or the pool's input when `lazy`."""
        K, Cin, kH, kW = self.weight.size()
        H, W = self.prevInput.size(-2), self.prevInput.size(-1)
        dev = src.device
        sp = self._split_workspace(work, H, W, dev)
        wp, scale = self._split_weights(H, W)
        prev = self.prevInput
        stateKey = (prev.data_ptr(), prev._version)
        rebuilt = sp['stateKey'] != stateKey
        if rebuilt:
            # first frame, or prevInput was (re)allocated or written by somebody else (restored states,
            # eval03.py:88-95): the pre-split copy is made again from it
            flag = () if sp['arith'] == 'x3' else (ptr(sp['flag']),)
            rebuild = C.cbinfer_split3_state_rebuild if sp['arith'] == 'x3' else C.cbinfer_split_state_rebuild
            check(rebuild(ptr(prev), ptr(sp['S']), Cin, H, W, kH, kW, *flag, stream_ptr(src)))
            sp['stateKey'] = stateKey
        pmask = lazy.producerMask() if (lazy is not None and self._pmask_ok(rebuilt)) else None
        q = self._fill_seq(sp, work, src, pmask)
        # what every entry point of the family takes, by the header's parameter names ...
        conv = dict(seqs=sp['seq'], nSeq=1, prepared=ptr(wp), bias=ptr(self.bias.detach()), C=Cin, H=H, W=W, K=K, kH=kH,
                    kW=kW, weightScale=float(scale), relu=int(bool(self.withReLU)), workspace=ptr(sp['ws']),
                    stream=stream_ptr(src))
        # ... and what the frame's detection adds (mode: bit 0 = behind a folded pool, bit 1 = not in feedback mode -- both
        # states take every value of the frame)
        frame = dict(conv, mode=int(lazy is not None) | (0 if self.feedbackLoop else 2),
                     pH=src.size(-2) if lazy is not None else 0, pW=src.size(-1) if lazy is not None else 0,
                     threshold=float(self.threshold))
        # the fused 1x1 tail behind this layer (pycbinfer.fuseTail1x1) rides in the contraction's second launch
        tail = self._folded_tail(sp, H, W, dev)
        # with a split-state consumer behind a lazy pool, the contraction in window order is its detection as well
        nextEligible, nxt, ntok, rawTok = self._window_fold(sp, tail, H, W)
        # fn(*args): the frame.  cfn(*cargs): the contraction alone (cbinfer_split_conv[_tail, _next]), for the frames whose
        # detection the PRODUCING layer's launch has done already (cb_rowpair.hip; its change indexes carry this layer's token)
        # sfn(*sargs): the contraction alone with a side job (round 6: the row-pair layer in front left its state refresh to this
        # launch's idle workgroups)
        side = sp.get('side') or sp.setdefault('side', _lib.SideRefresh())
        sfn, sargs = None, None
        if tail is not None:
            fn, cfn = C.cbinfer_split_forward_tail, C.cbinfer_split_conv_tail
            more = dict(forceSplit=0, tail=ctypes.pointer(sp['tail']))
            args, cargs = list(fn.pack(**frame, **more)), list(cfn.pack(**conv, **more))
        elif nxt is not None:
            fn, cfn, sfn = C.cbinfer_split_forward_next, C.cbinfer_split_conv_next, C.cbinfer_split_conv_next_refresh
            more = dict(next=ctypes.pointer(nxt))
            args, cargs = list(fn.pack(**frame, **more)), list(cfn.pack(**conv, **more))
            sargs = list(sfn.pack(side=ctypes.pointer(side), **conv, **more))
        else:
            fn, cfn = C.cbinfer_split_forward, C.cbinfer_split_conv
            args, cargs = list(fn.pack(**frame)), list(cfn.pack(forceSplit=0, **conv))
            if sp['arith'] == 'x3' and C.cbinfer_split_refresh_supported(Cin, K, kH, kW, H, W):      # (pixel order)
                sfn = C.cbinfer_split_conv_refresh
                sargs = list(sfn.pack(side=ctypes.pointer(side), **conv))
        token = self._split_token(sp, prev)
        done = lazy is not None and not rebuilt and getattr(lazy.indexes, 'nextDetect', None) == token
        pend = self.__dict__.get('_sidePending')
        if pend is not None and done and sargs is not None:
            self.__dict__.pop('_sidePending')
            side.frame, side.state, side.C, side.H, side.W, side.threshold = (ptr(pend[0]), ptr(pend[1]), pend[2], pend[3],
                                                                              pend[4], pend[5])
            check(sfn(*sargs))
        else:
            check(cfn(*cargs) if done else fn(*args))
        self._poll_range(sp)
        self.__dict__['_ranSplit'] = True
        self._inputIsLiveState = False
        self._lastIndexes = MaskChangeIndexes(sp['copy'], (H, W), work['idx'], work['count'], made=True)
        self._lastIndexes.tailDone = tail
        self._lastIndexes.nextDetect = ntok
        self._make_plan(lazy is not None, src, fn, args, None, pmask=ptr(pmask))
        if self._plan is not None:
            self._plan.update(
                split=True, arith=sp['arith'], switches=_split_switches(), checkPmask=True, stateVersion=prev._version,
                seq=q, indexes=self._lastIndexes, tail=tail, tailKey=tail._fold_key() if tail is not None else None,
                tailCand=self._fusedTailCandidate(), convFn=cfn, convArgs=cargs, detectToken=token,
                nextEligible=nextEligible, nextToken=ntok, nextRaw=rawTok, keep=nxt, hw=(H, W), side=side,
                sideFn=sfn, sideArgs=sargs)
        return self._emit(self._lastIndexes)

    def _run_split_plan(self, plan, inp, src):
        """The split-state plan's own conditions and per-frame arguments (_plan_source has checked the common ones)."""
        if plan['switches'] != _split_switches():
            return None      # (the arithmetic, or whether the layer runs on these kernels at all, may have changed)
        if not self._tail_unchanged(plan):
            return None
        if plan['nextEligible'] and self._next_detect(*plan['hw'])[1] != plan['nextRaw']:
            return None      # (the consumer's state or threshold is not the one this plan folds -- or it can fold now)
        if (plan['keep'] is not None and self.__dict__.get('_winFold', 'auto') == 'auto' and
                self.__dict__.get('_winAuto', {}).get('fold') is None and not torch.cuda.is_current_stream_capturing()):
            return None      # ('auto' has not seen a typical frame yet: the plan is made again, with another look)
        plan['seq'].input = src.data_ptr()
        if plan['pooled'] and getattr(inp.indexes, 'nextDetect', None) == plan['detectToken']:
            pend = self.__dict__.get('_sidePending')
            if pend is not None and plan['sideArgs'] is not None:
                # (the row-pair layer in front left its state refresh to this launch's idle workgroups)
                self.__dict__.pop('_sidePending')
                side = plan['side']
                key = (pend[1].data_ptr(),) + pend[2:]
                if plan.get('sideKey') != key:      # (everything but the frame's address stays from frame to frame)
                    side.state, side.C, side.H, side.W, side.threshold = key
                    plan['sideKey'] = key
                side.frame = pend[0].data_ptr()
                status = plan['sideFn'](*plan['sideArgs'])
            else:
                status = plan['convFn'](*plan['convArgs'])      # (the producing layer's launch was this frame's detection)
        else:
            status = plan['fn'](*plan['args'])
        if status != 0:
            check(status)
        self._poll_range(plan['work']['split'])
        self._inputIsLiveState = False
        return self._emit(plan['indexes'])

    def _workspace(self, input, wantMap=None):
        H, W = input.size(-2), input.size(-1)
        wantMap = self.saveChangeMap if wantMap is None else wantMap
        selfc = not wantMap and self._selfc_ok(H, W)      # (self-compacting, and no int8 copy of the mask wanted)
        key = (H, W, input.device, selfc)
        if self._work is None or self._work['key'] != key:
            dev = input.device
            # split-K workspace of the contraction kernel: owned by the module (kept across a change of
            # the frame size), so graphs and call plans of different modules or sequences never share
            # one, whatever stream they are captured or replayed on
            conv = self._work['conv'] if (self._work is not None and self._work['key'][2] == dev) \
                else newConvWorkspace(dev)
            nbytes = C.cbinfer_frame_mask_bytes(H, W) if selfc else 8 * C.cbinfer_mask_words(H, W)
            self._work = dict(
                key=key, selfc=selfc,
                bits=torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=dev),
                idx=torch.empty(H * W, dtype=torch.int32, device=dev),
                count=torch.zeros(1, dtype=torch.int32, device=dev),
                conv=conv, map=None, rows=None, split=None)      # (rows, split: _rows_workspace, _split_workspace)
        if wantMap and self._work['map'] is None:
            self._work['map'] = torch.zeros(H, W, dtype=torch.int8, device=input.device)
        return self._work

    # ---------------------------------------------------------------- fine-grained
    # Fine-grained frames (_path): by default per-value detection + accumulating fused contraction, no atomics, no host
    # sync; atomicFG: the reference-structured op sequence (f32 atomics).  fgInPlace updates the module's own tensors
    # in place (prevOutput and its relu'd copy alias the state across frames; capturable); without it, as the
    # reference does, fresh tensors are handed out and the caller's input is kept as state (conv2d.py:169-175).
    def _fg_workspace(self, x):
        """(work buffers, the relu'd copy of prevOutput an in-place frame keeps up to date or None)."""
        work = self._workspace(x, wantMap=False)     # (saveChangeMap has no meaning in fine-grained mode)
        assert work['selfc']
        if work.get('delta') is None or work['delta'].shape != x.shape:
            work['delta'] = torch.empty_like(x)
            work['relu'] = None
        if not (self.fgInPlace and self.withReLU):
            return work, None
        if work['relu'] is None:
            work['relu'] = F.relu(self.prevOutput)
        return work, work['relu']

    def _forward_fg_split(self, src, lazy, H, W, work, relu):
        """The fine-grained in-place frame on the split-state kernels: the detection leaves the thresholded differences
        in the pixel-major records, the contraction adds W * delta to prevOutput at the mask's pixels.  `lazy`: behind a
        folded CBPoolMax2d, `src` is the pool's input and H x W the pooled size."""
        K, Cin, kH, kW = self.weight.size()
        sp = self._split_workspace(work, H, W, src.device)
        wp, scale = self._split_weights(H, W)
        q = self._fill_seq(sp, work, src, None)
        q.delta, q.reluOut = work['delta'].data_ptr(), ptr(relu)
        sp['stateKey'] = None      # (the records hold differences now: a coarse-grained frame re-splits the state)
        pooled = lazy is not None
        args = [sp['seq'], 1, int(pooled), src.size(-2) if pooled else 0, src.size(-1) if pooled else 0, ptr(wp),
                Cin, H, W, K, kH, kW, float(self.threshold), float(scale), ptr(sp['ws'])]
        # the fused 1x1 tail behind this layer rides in the contraction's second launch, as in coarse-grained mode
        # (round 5: cbinfer_split_forward_fg_tail); it reads the relu'd copy when the layer has one
        tail = self._folded_tail(sp, H, W, src.device)
        if tail is not None and (not self.withReLU or relu is not None):
            fn = C.cbinfer_split_forward_fg_tail
            args += [ctypes.pointer(sp['tail']), stream_ptr(src)]
        else:
            tail, fn = None, C.cbinfer_split_forward_fg
            args += [stream_ptr(src)]
        check(fn(*args))
        self._poll_range(sp)
        self.__dict__['_ranSplit'] = True
        indexes = MaskChangeIndexes(sp['copy'], (H, W), work['idx'], work['count'], made=True)
        indexes.tailDone = tail
        result = self._emit(indexes, relu if self.withReLU else None)
        self._make_plan(pooled, src, fn, args, None, result=result)
        if self._plan is not None:
            self._plan.update(fgSplit=True, arith=sp['arith'], seq=q, wsplit=(wp, scale), relu=relu,
                              tail=tail, tailKey=tail._fold_key() if tail is not None else None,
                              tailCand=self._fusedTailCandidate())
        return result

    def forward_fg(self, inp):
        if isinstance(inp, LazyPool):
            # (behind a folded CBPoolMax2d: the in-place split-state frame takes the pool's input, the rest pools first)
            src, (H, W) = inp.source.detach(), inp.outSize[-2:]
            if self._path(src, H, W, pooled=True) == 'fg-split':
                if not self.prevInput.is_contiguous():
                    self.prevInput = self.prevInput.contiguous()
                work, relu = self._fg_workspace(self.prevInput)
                return self._forward_fg_split(src, inp, H, W, work, relu)
            inp = inp.tensor()
        x = inp.detach()
        K, Cin, kH, kW = self.weight.size()
        H, W = x.size(-2), x.size(-1)
        if self.prevInput.size() != x.size():
            # first frame / new size: dense convolution incl. bias (conv2d.py:163-167)
            self.prevOutput = F.conv2d(x, self.weight.detach(), bias=self.bias.detach(),
                                       padding=(kH // 2, kW // 2))
            self.prevInput = x.clone() if (self.fgInPlace and x.is_cuda) else x
            if self._work is not None:
                self._work['relu'] = None
            first = F.relu(self.prevOutput) if self.withReLU else self.prevOutput
            if not (self.propChangeIndexes and x.is_cuda):
                return first
            # (every output pixel is new on the first frame)
            return self._emit(torch.arange(H * W, dtype=torch.int32, device=x.device), first, last=False)
        x = x.contiguous()
        path = self._path(x, H, W)
        inplace = self.fgInPlace and path not in ('fg-det', 'fg-atomic')
        po = None if inplace else self.prevOutput.clone()           # conv2d.py:169
        indexes = None
        if path == 'fg-det':
            po = cbconvFG_deterministic(x, self.prevInput, po, self.weight.detach(), self.threshold,
                                        weightsPrepared=self._prepared_weights(H, W))
        elif path == 'fg-atomic':
            po = cbconvFG(x, self.prevInput, po, self.weight.detach(), self.threshold)
        else:
            work, relu = self._fg_workspace(x)
            if inplace:
                if not self.prevInput.is_contiguous():
                    self.prevInput = self.prevInput.contiguous()
                if path == 'fg-split':
                    return self._forward_fg_split(x, None, H, W, work, relu)
                return self._forward_fg_fused(x, path, work, self.prevInput, self.prevOutput, relu)
            indexes = self._forward_fg_fused(x, path, work, self.prevInput.contiguous(), po, None)
        self.prevOutput = po
        self.prevInput = x                                           # conv2d.py:175
        outp = F.relu(po) if self.withReLU else po
        if not (self.propChangeIndexes and x.is_cuda):
            return outp
        if indexes is None:
            # the atomic / deterministic forms keep no list of the pixels they touched: hand on EVERY pixel, so that a
            # consumer fed by the tuple protocol stays correct
            indexes = torch.arange(H * W, dtype=torch.int32, device=x.device)
        return self._emit(indexes, outp, last=False)

    def _forward_fg_fused(self, x, path, work, prev, out, relu):
        """A fine-grained frame on the mask-driven ('fg-rows', 'fg-blocks') or the list contraction ('fg-list'): in place
        (fgInPlace: `out` is prevOutput, `relu` its relu'd copy; returns the frame's result and keeps a call plan) or
        into `out`, a fresh copy of it (returns the change indexes)."""
        K, Cin, kH, kW = self.weight.size()
        H, W = x.size(-2), x.size(-1)
        inplace = self.fgInPlace
        if path == 'fg-list':
            arith = self._arith(x)
            fn, srcSlot = C.cbinfer_cbconv2d_forward_fg, 0
            args = (ptr(x), ptr(prev), ptr(work['delta']), ptr(out), ptr(relu), ptr(work['bits']), ptr(work['idx']),
                    ptr(work['count']), ptr(self._prepared_weights(H, W, arith)), Cin, H, W, K, kH, kW,
                    float(self.threshold), int(inplace), ptr(work['conv']), arith, stream_ptr(x))
            indexes = ChangeIndexes(work['idx'], work['count'], (H, W))
        else:
            rows = self._rows_workspace(work, H, W, x.device)
            fn, srcSlot = C.cbinfer_cbconv2d_forward_fg_masked, 1
            args = (int(path == 'fg-blocks'), ptr(x), ptr(prev), ptr(work['delta']), ptr(out), ptr(relu),
                    ptr(rows['bits']), ptr(rows['arrive']), ptr(rows['copy']), ptr(self._masked_call(path[3:])[1]),
                    Cin, H, W, K, kH, kW, float(self.threshold), int(inplace), stream_ptr(x))
            indexes = MaskChangeIndexes(rows['copy'], (H, W), work['idx'], work['count'])
        check(fn(*args))
        if not inplace:
            return indexes
        # (extension: the reference's forward_fg hands no indexes on)
        result = self._emit(indexes, relu if self.withReLU else None, last=path != 'fg-list')
        self._make_plan(False, x, fn, args, srcSlot, result=result, rows=path != 'fg-list')
        return result

    # ---------------------------------------------------------------- coarse-grained
    def _path(self, x, H, W, pooled=False, have=False):
        """Which kernel family runs this frame, from what it offers: the source `x` (behind a lazy pool, the pool's
        input), the layer's size H x W, a folded lazy pool or not, propagated change indexes or not, and the mode:
          coarse-grained  'split' / 'hsplit' (fp32 / fp16 split-state kernels), 'pairs' (cb_rowpair.hip), 'rows' /
                          'blocks' (mask-driven, _rows_path), 'list' (cb_conv.hip), 'ops' (the reference's op sequence)
          fine-grained    'fg-split', 'fg-rows', 'fg-blocks', 'fg-list', 'fg-det' (deterministicFG), 'fg-atomic'
          'dense'         behind a lazy pool: pool densely first.
          'geom'          a general-geometry layer (cb_geomconv.hip; H x W is its INPUT map); 'dense' behind a lazy pool"""
        dtype = x.dtype
        if self.__dict__.get('_geom'):
            if self.finegrained:
                raise _lib.CBinferError("CBConv2d: the fine-grained frame is not available on a general-geometry layer "
                                        "(kernel_size=%s stride=%s padding=%s dilation=%s%s)"
                                        % (tuple(self.kernel_size), tuple(self.stride), tuple(self.padding),
                                           tuple(self.dilation), '' if self.bias is not None else ', no bias'))
            return 'dense' if pooled else 'geom'
        if self.finegrained:
            fused = x.is_cuda and not self.atomicFG and dtype == torch.float32 and self._selfc_ok(H, W)
            if pooled:
                return 'fg-split' if (fused and self.fgInPlace and x.is_contiguous() and
                                      tuple(self.prevInput.size()) == (1, x.size(-3), H, W) and
                                      self._split_fg_ok(dtype, H, W)) else 'dense'
            if fused:
                if self.fgInPlace and self._split_fg_ok(dtype, H, W):
                    return 'fg-split'
                return 'fg-' + (self._rows_path(dtype, H, W) or 'list')
            return 'fg-det' if (x.is_cuda and self.deterministicFG and not self.atomicFG) else 'fg-atomic'
        if pooled:
            if (not self._selfc_ok(H, W) or dtype != self.weight.dtype or self.syncIndexes or self.saveChangeMap or
                    self.gatherComputationStats):
                return 'dense'
        elif self.syncIndexes:
            return 'ops'
        elif have or self.saveChangeMap or not self._selfc_ok(H, W):
            return 'list'
        if self._split_ok(dtype, H, W):
            return 'split'
        if self._hsplit_ok(dtype, H, W):
            return 'hsplit'
        if pooled and not self.feedbackLoop:      # (the other pooled frames refresh the state at the changed pixels only)
            return 'dense'
        path = self._rows_path(dtype, H, W)
        if path == 'rows' and not pooled and self._pairs_ok(H, W):
            return 'pairs'
        return path or 'list'

    def _selfc_ok(self, H, W):
        """The self-compacting frame (detection + fused contraction, no compaction launch) takes an H x W mask."""
        return C.cbinfer_mask_words(H, W) <= C.cbinfer_frame_mask_max_words() and not _switch('CBINFER_NO_SELFCOMPACT')

    def _pmask_ok(self, fresh):
        """May this frame's detection skip what the producer's change mask leaves out?  Not on a fresh or restored state,
        nor after a change of the threshold (the skipped segments compared below THIS threshold last frame)."""
        th = float(self.threshold)
        same = self.__dict__.get('_pmaskThreshold') == th
        self.__dict__['_pmaskThreshold'] = th
        return same and not fresh

    def _emit(self, indexes, out=None, last=True):
        """A frame's result: `out` (default prevOutput), a tuple with propChangeIndexes; `last`: lastChangeIndexes()"""
        if last:
            self._lastIndexes = indexes
        if out is None:
            out = self._buffers['prevOutput']
        return ('changeIndexes', out, indexes) if self.propChangeIndexes else out

    def forward_normal(self, inp):
        # input parsing and checks (conv2d.py:180-190)
        changeIndexes = None
        if self.__dict__.get('_geom'):
            return self._forward_geom(inp)
        if isinstance(inp, LazyPool):
            path = self._path(inp.source, inp.outSize[-2], inp.outSize[-1], pooled=True)
            if path != 'dense':
                return self._forward_pooled(inp, path)
            inp = inp.tensor()
        src = inp[1] if type(inp) == tuple else inp
        # a producer that hands out its in-place-updated state (CBPoolMax2d.cloneOutput=False) tags it
        self._inputIsLiveState = bool(getattr(src, '_cbinfer_inplace_state', False))
        input = src.detach().contiguous()
        if type(inp) == tuple:
            assert inp[0] == 'changeIndexes'
            changeIndexes = inp[2]
            if isinstance(changeIndexes, torch.Tensor):
                changeIndexes = changeIndexes.detach().contiguous()
            assert changeIndexes.dim() == 1
        assert input.size(-3) == self.in_channels
        assert input.dim() == 4 and input.size(0) == 1
        require_device(input)
        assert input.dtype == self.weight.dtype, "input and weights must have the same dtype"
        if (changeIndexes is not None and self.dilatePropagatedIndexes and
                (self.weight.size(2) > 1 or self.weight.size(3) > 1)):
            size = (input.size(-2), input.size(-1))
            if isinstance(changeIndexes, ChangeIndexes) and changeIndexes.size not in (None, size):
                raise _lib.CBinferError("CBConv2d: the propagated change indexes address a %dx%d map, this layer "
                                        "runs at %dx%d" % (changeIndexes.size + size))
            dilated = dilateChangeIndexes(changeIndexes, size, (self.weight.size(2), self.weight.size(3)))
            # (the reference-structured mode hands exact tensors on, conv2d_cg.py:207)
            changeIndexes = dilated.tensor().clone() if self.syncIndexes else dilated

        self._state_for(input.size(), input)

        if self.gatherComputationStats:
            self._gatherStats(input)

        path = self._path(input, input.size(-2), input.size(-1), have=changeIndexes is not None)
        if path != 'ops':
            return self._forward_fused(input, changeIndexes, path)
        changeIndexes = self._forward_ops(input, changeIndexes)
        self._lastIndexes = (changeIndexes if isinstance(changeIndexes, ChangeIndexes) else
                             ChangeIndexes(changeIndexes, torch.tensor([changeIndexes.numel()],
                                                                      dtype=torch.int32, device=input.device),
                                           (input.size(-2), input.size(-1))))
        return self._emit(changeIndexes, last=False)

    def _state_for(self, size, like):
        """(Re)allocate the state, +inf: a first frame is 100 % change (conv2d.py:192-199).  -> prevInput is new
        (prevOutput of a general-geometry layer with output pixels no tap reaches: _bias_map)"""
        fresh = (tuple(self.prevInput.size()) != tuple(size) or self.prevInput.dtype != like.dtype or
                 self.prevInput.device != like.device)
        if fresh:
            self.prevInput = torch.full(size, float('inf'), dtype=like.dtype, device=like.device)
        outpSize = list(size)
        outpSize[-3] = self.out_channels
        outpSize[-2], outpSize[-1] = self._out_hw(size[-2], size[-1])
        if (not _same_shape(self.prevOutput, outpSize) or self.prevOutput.dtype != like.dtype or
                self.prevOutput.device != like.device):
            if self._has_unreached_outputs():
                self.prevOutput = self._bias_map(outpSize, like)
            else:
                self.prevOutput = torch.full(outpSize, float('inf'), dtype=like.dtype, device=like.device)
        return fresh

    def _has_unreached_outputs(self):
        """Padding beyond the dilated filter's reach on an axis (p > d (k-1), nn.Conv2d(3, 8, 3, padding=3)): the outer
        output pixels have no tap inside the input map, so no frame ever lists or writes them."""
        if not self.__dict__.get('_geom'):
            return False
        k, p, d = self.kernel_size, self.padding, self.dilation
        return any(p[i] > d[i] * (k[i] - 1) for i in (0, 1))

    def _bias_map(self, size, like):
        """The dense value of an output pixel without an in-map tap, broadcast over the map: the bias (0 without one),
        after the ReLU when withReLU -- exact in fp32 and fp16.  Made when the state is (re)allocated, with the flags of
        that moment: the first frame overwrites every reachable pixel, the others keep this value until the next
        clearMemory() or change of resolution / dtype / device -- so a withReLU toggled in the middle of a sequence
        reaches them as it reaches any unlisted pixel, not at all."""
        fill = torch.zeros(size, dtype=like.dtype, device=like.device)
        if self.bias is not None:
            b = self.bias.detach().to(device=like.device, dtype=like.dtype)
            fill += (F.relu(b) if self.withReLU else b).view(1, -1, 1, 1)
        return fill

    def _forward_pooled(self, lazy, path):
        """A layer behind a lazy CBPoolMax2d (pycbinfer.fusePoolingIntoDetection) on `path` (_path): its change detection
        takes the 2x2 max of the pool's input on the fly (cbinfer_cbconv2d_forward_pooled and its kin)."""
        src = lazy.source.detach().contiguous()
        size = lazy.outSize
        H, W = size[-2], size[-1]
        assert size[-3] == self.in_channels and src.dim() == 4 and src.size(0) == 1
        require_device(src)
        fresh = self._state_for(size, src)
        self._inputIsLiveState = False
        work = self._workspace(self.prevInput)
        if path == 'split':
            return self._forward_split(src, lazy, work)
        if path == 'hsplit':
            return self._forward_hsplit(src, work, lazy)
        if path != 'list':
            return self._emit(self._forward_masked(src, work, path, lazy, fresh))
        K, Cin, kH, kW = self.weight.size()
        arith = self._arith(src)
        args = (ptr(src), src.size(-2), src.size(-1), ptr(self.prevInput), ptr(self.prevOutput),
                ptr(work['bits']), ptr(work['idx']), ptr(work['count']),
                ptr(self._prepared_weights(H, W, arith)), ptr(self.bias.detach()), Cin, H, W, K, kH, kW,
                float(self.threshold), int(bool(self.withReLU)), ptr(work['conv']), arith, stream_ptr(src))
        check(C.cbinfer_cbconv2d_forward_pooled(*args))
        self._make_plan(True, src, C.cbinfer_cbconv2d_forward_pooled, args, 0)
        return self._emit(ChangeIndexes(work['idx'], work['count'], (H, W)))

    def _forward_fused(self, input, changeIndexes, path):
        """One library call per frame on `path` (_path): no host sync (see cbinfer_cbconv2d_forward)."""
        work = self._workspace(input)
        if not self.prevInput.is_contiguous():
            self.prevInput = self.prevInput.contiguous()
        if path == 'split':
            return self._forward_split(input, None, work)
        if path == 'hsplit':
            return self._forward_hsplit(input, work)
        if path == 'pairs':
            result = self._forward_pairs(input, work)
        elif path == 'list':
            result = self._forward_list(input, changeIndexes, work)
        else:
            result = self._forward_masked(input, work, path)
        if not self.feedbackLoop and not self.copyInput:
            # alias, conv2d.py:237-238 (a producer's in-place-updated state is copied first)
            self.prevInput = input.clone() if self._inputIsLiveState else input
        return self._emit(result)

    def _forward_masked(self, src, work, path, lazy=None, fresh=False):
        """A frame on a mask-driven contraction ('rows' / 'blocks'); `lazy`: behind a folded pool (`src` is its input,
        `fresh`: the state was just allocated).  Returns the indexes."""
        K, Cin, kH, kW = self.weight.size()
        H, W = self.prevInput.size(-2), self.prevInput.size(-1)
        rows = self._rows_workspace(work, H, W, src.device)
        fn, wprep = self._masked_call(path)
        if lazy is None:
            pmask, head = None, (ptr(src), None, 0, 0, None)
        else:
            pmask = lazy.producerMask() if self._pmask_ok(fresh) else None
            head = (None, ptr(src), src.size(-2), src.size(-1), ptr(pmask))
        args = head + (ptr(self.prevInput), ptr(self.prevOutput), ptr(rows['bits']), ptr(rows['arrive']),
                       ptr(rows['copy']), ptr(wprep), ptr(self.bias.detach()), Cin, H, W, K, kH, kW,
                       float(self.threshold), int(bool(self.feedbackLoop)), int(lazy is None and bool(self.copyInput)),
                       int(bool(self.withReLU)), stream_ptr(src))
        check(fn(*args))
        if not self._inputIsLiveState:
            self._make_plan(lazy is not None, src, fn, args, int(lazy is not None), rows=True, pmask=ptr(pmask))
        return MaskChangeIndexes(rows['copy'], (H, W), work['idx'], work['count'])

    def _forward_pairs(self, input, work):
        """The row-pair kernel: persistent over the non-empty units, and -- with a split-state consumer behind a lazy pool
        (pycbinfer.fuseDetectionIntoProducer) -- that consumer's pooled change detection in the same launch."""
        K, Cin, kH, kW = self.weight.size()
        H, W = input.size(-2), input.size(-1)
        prev = self.prevInput
        rows = self._rows_workspace(work, H, W, input.device)
        _, wprep = self._masked_call('rows')
        nxt, tok = self._next_detect(H, W)
        det = self._pair_detect_ok(nxt, kH)
        if det:
            # round 6: this layer's own detection inside the row-pair launch; the state is refreshed by the consumer's
            # contraction (or, failing that, by a launch of its own behind the consumer's: CBConv2d.forward)
            cons = self.__dict__['_fusedNext'][1]
            old = cons.__dict__.pop('_sidePending', None)
            if old is not None:      # (the consumer was not called last frame)
                _flush_side(old)
            fn = C.cbinfer_conv_rowpairs_detect
            args = (ptr(input), ptr(prev), ptr(self.prevOutput), ptr(rows['copy']), ptr(wprep),
                    ptr(self.bias.detach()), Cin, H, W, K, kH, kW, float(self.threshold), int(bool(self.withReLU)),
                    ctypes.pointer(nxt), stream_ptr(input))
            check(fn(*args))
            cons.__dict__['_sidePending'] = (input, prev, Cin, H, W, float(self.threshold))      # (tensors: kept alive)
        else:
            fn = C.cbinfer_cbconv2d_forward_rowpairs
            args = (ptr(input), ptr(prev), ptr(self.prevOutput), ptr(rows['bits']), ptr(rows['arrive']),
                    ptr(rows['copy']), ptr(wprep), ptr(self.bias.detach()), Cin, H, W, K, kH, kW,
                    float(self.threshold), int(bool(self.withReLU)),
                    ctypes.pointer(nxt) if nxt is not None else None, stream_ptr(input))
            check(fn(*args))
        result = MaskChangeIndexes(rows['copy'], (H, W), work['idx'], work['count'])
        result.nextDetect = tok
        if not self._inputIsLiveState:
            self._make_plan(False, input, fn, args, 0, rows=True)
            if self._plan is not None:
                self._plan.update(pairs=True, nextToken=tok, keep=nxt, det=det)
        return result

    def _forward_list(self, input, changeIndexes, work):
        """The list kernel (cb_conv.hip): this layer's own detection, or the propagated change indexes."""
        K, Cin, kH, kW = self.weight.size()
        H, W = input.size(-2), input.size(-1)
        have = changeIndexes is not None
        if have and self.feedbackLoop:
            # the reference skips detection here and so never refreshes prevInput (conv2d.py:220-238):
            # its gather would read the +inf initial state.  Refuse instead of computing garbage.
            raise _lib.CBinferError("CBConv2d: feedbackLoop=True cannot be combined with propagated "
                                    "change indexes (the layer state would never be updated)")
        if have:
            if isinstance(changeIndexes, ChangeIndexes):
                idx, count, cap = changeIndexes.buffer, changeIndexes.count, changeIndexes.buffer.numel()
                if changeIndexes.size is not None and changeIndexes.size != (H, W):
                    raise _lib.CBinferError(
                        "CBConv2d: the propagated change indexes address a %dx%d map, this layer runs at "
                        "%dx%d (a CBPoolMax2d in between must hand on down-sampled indexes: "
                        "downsampleIndexes=True)" % (changeIndexes.size + (H, W)))
            else:
                idx, cap = changeIndexes, changeIndexes.numel()
                count = None
            if idx.dtype != torch.int32 or not idx.is_contiguous():
                raise _lib.CBinferError("CBConv2d: propagated change indexes must be a contiguous int32 "
                                        "tensor (conv2d_cg.py:207: nonzero(...).int())")
            cap = min(cap, H * W)
            result = changeIndexes
            if count is None:
                # exact host-side list: write its length where the kernels look for it
                count = torch.full((1,), cap, dtype=torch.int32, device=input.device)
        else:
            idx, count, cap = work['idx'], work['count'], H * W
            result = ChangeIndexes(idx, count, (H, W))
            if work['selfc'] and not self.saveChangeMap:
                # (round 6: the self-compacting contraction leaves a copy of the frame's change mask at a fixed address
                #  inside the frame mask buffer -- a chained consumer's detection skips the segments this layer left alone)
                off = C.cbinfer_frame_mask_copy_offset(H, W) // 8
                result = MaskChangeIndexes(work['bits'][off:off + C.cbinfer_mask_words(H, W)], (H, W), idx, count,
                                           made=True)
        mapOut = work['map'] if (self.saveChangeMap and not have) else None
        if cap > 0:
            arith = self._arith(input)
            frame = dict(input=ptr(input), prevInput=ptr(self.prevInput), prevOutput=ptr(self.prevOutput),
                         bits=None if have else ptr(work['bits']), idx=ptr(idx), countDev=ptr(count),
                         weightsPrepared=ptr(self._prepared_weights(H, W, arith)), bias=ptr(self.bias.detach()), C=Cin, H=H,
                         W=W, K=K, kH=kH, kW=kW, threshold=float(self.threshold), feedbackLoop=int(bool(self.feedbackLoop)),
                         copyInput=int(bool(self.copyInput)), relu=int(bool(self.withReLU)), workspace=ptr(work['conv']),
                         dtype=arith, stream=stream_ptr(input))
            # (the parameter order is asked of the binding itself: this module's C may be a wrapper that notes the calls --
            #  the tests' spies hand out plain functions -- and the call below must still go through it)
            args = _lib.C.cbinfer_cbconv2d_forward.pack(mapOut=ptr(mapOut), haveIndexes=int(have), capN=cap,
                                                        selfCompact=int(work['selfc'] and not have), **frame)
            check(C.cbinfer_cbconv2d_forward(*args))
            if not have and not self._inputIsLiveState:
                if work['selfc'] and mapOut is None:
                    # replayed through the chained entry: a frame in which the layer that produced `input` rewrote
                    # nothing ends both launches at once (_upstream_count decides per frame whether that may be said)
                    cargs = _lib.C.cbinfer_cbconv2d_forward_after.pack(upstreamCount=None, **frame)
                    self._make_plan(False, input, C.cbinfer_cbconv2d_forward_after, cargs, 1)
                    if self._plan is not None:
                        self._plan['chain'] = True
                        self._plan['indexes'] = result
                else:
                    self._make_plan(False, input, C.cbinfer_cbconv2d_forward, args, 0)
            if work['selfc'] and not have:
                self._publish_count(work['count'])
        if mapOut is not None:
            # (a view of the module's work buffer, rewritten by the next frame -- clone it to keep it; the
            #  reference allocates a fresh map per frame)
            self.changeMap = mapOut
        return result

    def _forward_ops(self, input, changeIndexes):
        """The reference's op sequence (conv2d.py:220-251), one kernel launch per op, blocking on the
        change count like torch.nonzero does."""
        if isinstance(changeIndexes, ChangeIndexes):
            changeIndexes = changeIndexes.tensor()
        if changeIndexes is None:
            changeMap = changeDetection(input, self.prevInput, self.kernel_size, self.threshold,
                                        updateInputState=self.feedbackLoop)
            if self.saveChangeMap:
                self.changeMap = changeMap
            changeIndexes = changeIndexesExtr(changeMap)
        if not self.feedbackLoop:
            if self.copyInput:
                self.prevInput.copy_(input)
            else:
                self.prevInput = input.clone() if self._inputIsLiveState else input
        if changeIndexes.numel() != 0:
            Xmatrix = genXMatrix(self.prevInput, changeIndexes, self.kernel_size)
            Ymatrix = matrixMult(Xmatrix, self.weight.detach(), self.bias.detach(), transposeOut=True,
                                 weightsPrepared=self._prepared_weights())
            updateOutput(Ymatrix, changeIndexes, self.prevOutput, withReLU=self.withReLU)
        return changeIndexes

    def _gatherStats(self, input):
        """Operation counts behind the 'effective GOp/s' metric (conv2d.py:201-218)."""
        changeTensor = (input - self.prevInput).abs().gt(self.threshold)
        nC = changeTensor.size(-3)
        kH, kW = self.weight.size(2), self.weight.size(3)
        if self.__dict__.get('_geom'):
            # the footprint on the OUTPUT map: Ho x Wo values per feature map
            proped = F.conv2d(changeTensor.float(), torch.ones(nC, 1, kH, kW, device=input.device), stride=self.stride,
                              padding=tuple(self.padding), dilation=self.dilation, groups=nC).gt(0)
        else:
            proped = F.conv2d(changeTensor.float(),
                              torch.ones(nC, 1, kH, kW, device=input.device), groups=nC).gt(0)
        opsPerValue = self.weight.size(0) * kH * kW * 2
        self.compStats = dict(
            numInputChangesPerFeatureMap=changeTensor.sum() * opsPerValue,
            numInputChanges=changeTensor.sum(-3).gt(0).sum() * nC * opsPerValue,
            numInputPropedChangesPerFeatureMap=proped.sum() * opsPerValue,
            numInputPropedChanges=proped.sum(-3).gt(0).sum() * nC * opsPerValue,
            totalInputValues=proped.size(-1) * proped.size(-2) * nC * opsPerValue
            if self.__dict__.get('_geom') else changeTensor.size(-1) * changeTensor.size(-2) * nC * opsPerValue)

    # ---------------------------------------------------------------- per-frame fast path
    # After a frame went through the general path, its library call is kept as a plan -- a pre-built argument list plus
    # the facts that must still hold (_plan_source, and each path's own) -- and replayed while they hold: ~10 instead
    # of ~35 us of host time per layer and frame.
    def _flags(self):
        return (self.threshold, self.feedbackLoop, self.copyInput, self.withReLU, self.propChangeIndexes,
                self.syncIndexes, self.saveChangeMap, self.gatherComputationStats, self.finegrained,
                self.atomicFG, self.fgInPlace, self.exactF32, self.dilatePropagatedIndexes)

    def _make_plan(self, pooled, src, fn, args, srcSlot, result=None, rows=False, pmask=None):
        """Remember a finished sync-free call: fn(*args) with args[srcSlot] = source pointer, args[-1] =
        stream.  Only for configurations whose call does not depend on per-frame host state."""
        if self.syncIndexes or self.saveChangeMap or self.gatherComputationStats:
            return
        if not (self.feedbackLoop or self.copyInput or result is not None):
            return
        w, b = self._parameters.get('weight'), self._parameters.get('bias')
        if w is None or (b is None and not self.__dict__.get('_geom')) or _switch('CBINFER_NO_FASTPATH'):
            return
        work = self._work
        self._plan = dict(
            pooled=pooled, shape=tuple(src.shape), dtype=src.dtype, device=src.device, flags=self._flags(),
            w=(w.data_ptr(), w._version), b=(b.data_ptr(), b._version) if b is not None else None,
            state=(self._buffers['prevInput'].data_ptr(), self._buffers['prevOutput'].data_ptr()),
            stream=args[-1], work=work, fn=fn, args=list(args), srcSlot=srcSlot, result=result, rows=rows, pmask=pmask,
            indexes=ChangeIndexes(work['idx'], work['count'], work['key'][:2]))

    def _plan_source(self, inp):
        """The source tensor if the kept call plan applies to `inp` as it stands -- what every plan assumes; no side
        effects --, else None."""
        plan = self._plan
        if plan['pooled']:
            if type(inp) is not LazyPool:
                return None
            src = inp.source
            if plan['rows'] or plan.get('checkPmask'):      # the producer's mask is baked into the call: it must still be the one offered
                pm = inp.producerMask()
                if (pm.data_ptr() if pm is not None else None) != plan['pmask']:
                    return None
        else:
            if type(inp) is not torch.Tensor:
                return None
            src = inp
        w, b, bufs = self._parameters['weight'], self._parameters.get('bias'), self._buffers
        if (src.shape != plan['shape'] or src.dtype != plan['dtype'] or src.device != plan['device'] or
                not src.is_contiguous() or self._flags() != plan['flags'] or
                (w.data_ptr(), w._version) != plan['w'] or
                (None if b is None else (b.data_ptr(), b._version)) != plan['b'] or
                (bufs['prevInput'].data_ptr(), bufs['prevOutput'].data_ptr()) != plan['state'] or
                self._work is not plan['work'] or raw_stream(src.device.index) != plan['stream']):
            return None
        if plan.get('stateVersion') is not None and bufs['prevInput']._version != plan['stateVersion']:
            return None      # (somebody wrote prevInput through torch: its pixel-major copy must be made again)
        return src

    def _run_plan(self, inp):
        plan = self._plan
        src = self._plan_source(inp)
        if src is None:
            return None
        if plan.get('split'):
            return self._run_split_plan(plan, inp, src)
        bufs = self._buffers
        if plan.get('hsplit'):
            tokens = self._prepare_hsplit(plan, src, bufs)
            status = plan['fn'](*plan['args'])
            if status != 0:
                check(status)
            return self._finish_hsplit(plan, tokens, bufs)
        if plan.get('pairs'):
            # the next layer's detection rides in this launch: the plan holds only while that layer's state is the one
            # the plan was made for (and starts to fold as soon as it can)
            if self._next_detect(plan['shape'][-2], plan['shape'][-1])[1] != plan['nextToken']:
                return None
            if plan.get('det') != self._pair_detect_ok(plan['keep'], self.weight.size(2)):
                return None
            if plan.get('det'):
                cons = self.__dict__['_fusedNext'][1]
                old = cons.__dict__.pop('_sidePending', None)
                if old is not None:
                    _flush_side(old)
                cons.__dict__['_sidePending'] = (src, bufs['prevInput'], src.size(1), src.size(-2), src.size(-1),
                                                 float(self.threshold))
        args = plan['args']
        if plan.get('fgSplit'):
            if plan['arith'] != _switch('CBINFER_ARITH'):
                return None
            if not self._tail_unchanged(plan):
                return None
            plan['seq'].input = src.data_ptr()
        else:
            args[plan['srcSlot']] = src.data_ptr()
        chain = plan.get('chain')
        if chain:
            up = self.__dict__.get('_upNow')
            args[0] = up.data_ptr() if up is not None else None
        status = plan['fn'](*args)
        if status != 0:
            check(status)
        if chain:
            self._publish_count(plan['work']['count'])
        if plan.get('fgSplit'):
            self._poll_range(plan['work']['split'])
        self._inputIsLiveState = False
        res = plan['result']                    # (fine-grained in-place frame: prevOutput or its relu'd copy)
        if not plan['rows']:
            return self._emit(plan['indexes']) if res is None else res
        # mask-driven frame: the list is made from this frame's mask copy when somebody asks
        work = plan['work']
        indexes = MaskChangeIndexes(work['rows']['copy'], work['key'][:2], work['idx'], work['count'])
        if res is not None:
            return self._emit(indexes, res[1] if isinstance(res, tuple) else res)
        indexes.nextDetect = plan.get('nextToken')
        return self._emit(indexes)

    def _prepare_hsplit(self, plan, src, bufs):
        """The per-frame arguments of an fp16 split-state plan: input, the chain's count and mask, whose detection rides
        where.  Returns the consumers' tokens."""
        L, hs = plan['layer'], plan['hs']
        H, W = plan['size']
        L.input = src.data_ptr()
        up = self.__dict__.get('_upNow')
        L.upstreamCount = up.data_ptr() if up is not None else None
        if not plan['pooled']:
            pm = self._chain_mask(H, W)
            L.producerMask = pm.data_ptr() if pm is not None else None
            L.detect = 0 if self._detected_upstream(self._half_token(hs, bufs['prevInput'])) else 1
        return self._fill_consumers(L, H, W) if '_fusedConsumers' in self.__dict__ else ()

    def _finish_hsplit(self, plan, tokens, bufs):
        self.__dict__['_ranSplit'] = True
        self._publish_count(plan['work']['count'], tokens)
        self._inputIsLiveState = False
        return self._emit(plan['indexes'])

    # ---------------------------------------------------------------- chains of change-based layers
    # A layer whose self-compacting contraction ran tags its output buffer with where its change count is (_Produced).
    # The next CBConv2d handed this very buffer may pass that count to its launches (cbinfer_cbconv2d_forward_after):
    # zero there ends its frame at once.  Checked on the host every frame: the tag is of the producer's latest forward,
    # nobody wrote the buffer or this layer's state through torch since, and this layer's previous forward consumed
    # the producer's previous frame from the same buffer.  CBINFER_NO_CHAIN=1 switches it off.
    def _publish_count(self, count, tokens=()):
        out = self._buffers['prevOutput']
        out._cbProduced = _Produced(self, self.__dict__.get('_serial', 0), out._version, count, tokens)

    def _chain_mask(self, H, W):
        """The change mask the PRODUCING layer of a chain left this frame (its MaskChangeIndexes' mask copy, H x W) while
        the chain's conditions hold (_note_upstream: the input is that layer's output buffer of its latest frame, this
        layer consumed its previous one from the same buffer into the same state) -- else None.  CBINFER_NO_CHAINMASK=1
        switches it off."""
        d = self.__dict__
        if d.get('_upNow') is None or _switch('CBINFER_NO_CHAINMASK'):
            return None
        ix = getattr(d['_upSeen'][0], '_lastIndexes', None)
        if isinstance(ix, MaskChangeIndexes) and tuple(ix.size) == (H, W) and ix._mask is not None:
            return ix._mask
        return None

    def _note_upstream(self, inp):
        d = self.__dict__
        d['_serial'] = d.get('_serial', 0) + 1
        tag = getattr(inp, '_cbProduced', None) if type(inp) is torch.Tensor else None
        seen, now = None, None
        d['_upTokens'] = tag.tokens if tag is not None else None
        if tag is not None:
            prod, serial, version, count = tag.module, tag.serial, tag.version, tag.count
            pin = self._buffers.get('prevInput')
            if (prod is not self and prod.__dict__.get('_serial') == serial and inp._version == version and
                    pin is not None and not _NO_CHAIN):
                seen = (prod, serial, inp.data_ptr(), pin.data_ptr(), pin._version)
                last = d.get('_upSeen')
                if last is not None and last[0] is prod and last[1] == serial - 1 and last[2:] == seen[2:]:
                    now = count
        d['_upSeen'], d['_upNow'] = seen, now

    def forward(self, inp):
        out = self._forward(inp)
        # a row-pair layer in front that left its state refresh to this layer's contraction, which did not carry it
        pend = self.__dict__.pop('_sidePending', None)
        if pend is not None:
            _flush_side(pend)
        return out

    def _forward(self, inp):
        self._note_upstream(inp)
        if self.__dict__.get('_plan') is not None:
            out = self._run_plan(inp)
            if out is not None:
                return out
            self._plan = None
        self._setDefaultValues()
        self.__dict__['_ranSplit'] = False
        if self.finegrained:
            assert self.feedbackLoop == False
            if self.__dict__.get('_geom'):
                self._path(self.weight, 1, 1)      # (raises: no fine-grained frame on general geometry)
            out = self.forward_fg(inp)
        else:
            out = self.forward_normal(inp)
        if not self.__dict__['_ranSplit']:
            # a frame on any other path refreshes prevInput through raw pointers: the split copies of the state are
            # stale and are made again when the module returns to the split-state kernels
            for name in ('split', 'hsplit'):
                st = self._work.get(name) if self._work else None
                if st is not None:
                    st['stateKey'] = None
        return out

    def __repr__(self):
        """One line in the reference's format (conv2d.py:271-290): fixed head, then the conv attributes
        that differ from their defaults, then the change-based flags."""
        self._setDefaultValues()
        optional = [('pad', self.padding, (0,) * len(self.padding)),
                    ('dilation', self.dilation, (1,) * len(self.dilation)),
                    ('outpad', self.output_padding, (0,) * len(self.output_padding)),
                    ('grp', self.groups, 1)]
        parts = ['th=%s' % (self.threshold,), '%s->%s' % (self.in_channels, self.out_channels),
                 'k=%s' % (self.kernel_size,), 's=%s' % (self.stride,), 'copyInput=%s' % (self.copyInput,)]
        parts += ['%s=%s' % (label, value) for label, value, default in optional if value != default]
        if self.bias is None:
            parts.append('bias=False')
        if self.withReLU:
            parts.append('withReLU=%s' % (self.withReLU,))
        parts.append('propChgIdxs=%s' % (self.propChangeIndexes,))
        return '%s (%s)' % (self.__class__.__name__, ', '.join(parts))


class CBTail1x1(nn.Module):
    """conv1x1 -> [ReLU] -> conv1x1 evaluated in one launch at the pixels of the change list handed on by
    the CBConv2d in front of it (tuple protocol, conv2d.py:180-186); every other output pixel keeps its
    value.  Stands for two CBConv2d fed by propagated change indexes (sceneLabeling/modelLoader.py:41-44)
    or for the dense 1x1 tail the other experiments keep (:45-47); built by pycbinfer.fuseTail1x1().
    The parameters are shared with the source modules."""

    @staticmethod
    def maxHidden():
        return int(C.cbinfer_tail1x1_max_hidden())

    @staticmethod
    def supported(C0, C1, C2):
        """Channel counts the one-launch kernel takes (hidden width and its LDS budget)."""
        return bool(C.cbinfer_tail1x1_supported(int(C0), int(C1), int(C2)))

    @staticmethod
    def accepts(m):
        def pair(v):
            return tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        return (pair(m.kernel_size) == (1, 1) and pair(m.stride) == (1, 1) and pair(m.padding) == (0, 0) and
                pair(m.dilation) == (1, 1) and m.groups == 1 and m.bias is not None)

    def __init__(self, conv1, conv2, relu=True):
        super(CBTail1x1, self).__init__()
        assert CBTail1x1.accepts(conv1) and CBTail1x1.accepts(conv2)
        assert conv1.out_channels == conv2.in_channels
        if not CBTail1x1.supported(conv1.in_channels, conv1.out_channels, conv2.out_channels):
            raise _lib.CBinferError("CBTail1x1: %d->%d->%d channels exceed the kernel's hidden width or LDS budget"
                                    % (conv1.in_channels, conv1.out_channels, conv2.out_channels))
        self.weight1, self.bias1 = conv1.weight, conv1.bias
        self.weight2, self.bias2 = conv2.weight, conv2.bias
        self.in_channels, self.hidden_channels, self.out_channels = (
            conv1.in_channels, conv1.out_channels, conv2.out_channels)
        self.relu = bool(relu)
        self.withReLU = False
        self.propChangeIndexes = False
        self.register_buffer('prevOutput', torch.zeros(0))
        self._w1prep = None

    def clearMemory(self):
        self.prevOutput = self.weight1.detach().new_zeros(0)

    def getStateTensors(self):
        return [self.prevOutput]

    def __getstate__(self):
        d = dict(self.__dict__)
        d['_w1prep'] = None
        return d

    def _prepared(self):
        w = self.weight1
        key = (w.data_ptr(), w._version, w.device)
        if self._w1prep is None or self._w1prep[0] != key:
            nbytes = C.cbinfer_tail1x1_prepared_bytes(self.hidden_channels, self.in_channels)
            wp = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
            check(C.cbinfer_tail1x1_prep(ptr(w.detach().contiguous()), ptr(wp), self.hidden_channels,
                                         self.in_channels, stream_ptr(w)))
            self._w1prep = (key, wp)
        return self._w1prep[1]

    def _output_for(self, H, W, device, dtype):
        size = (1, self.out_channels, H, W)
        if not _same_shape(self.prevOutput, size) or self.prevOutput.device != device:
            self.prevOutput = torch.full(size, float('inf'), dtype=dtype, device=device)
        return self.prevOutput

    def _fold_key(self):
        """What a producing layer's call plan that folds this tail into its own launch depends on."""
        ts = (self.weight1, self.bias1, self.weight2, self.bias2)
        return (tuple((t.data_ptr(), t._version) for t in ts), self._buffers['prevOutput'].data_ptr(), self.relu,
                bool(self.withReLU))

    def forward(self, inp):
        assert type(inp) == tuple and inp[0] == 'changeIndexes', \
            "CBTail1x1 needs the ('changeIndexes', tensor, indexes) tuple of a CBConv2d with propChangeIndexes"
        if getattr(inp[2], 'tailDone', None) is self:
            # the producing layer evaluated this tail in its own second launch (cbinfer_split_forward_tail)
            if self.propChangeIndexes:
                return 'changeIndexes', self.prevOutput, inp[2]
            return self.prevOutput
        x, indexes = inp[1].detach().contiguous(), inp[2]
        require_device(x)
        assert x.dim() == 4 and x.size(0) == 1 and x.size(1) == self.in_channels
        if x.dtype != torch.float32:
            raise _lib.CBinferError("CBTail1x1 is fp32 only")
        H, W = x.size(-2), x.size(-1)
        self._output_for(H, W, x.device, x.dtype)
        if isinstance(indexes, ChangeIndexes):
            idx, count, cap = indexes.buffer, indexes.count, min(indexes.buffer.numel(), H * W)
        else:
            idx = indexes.detach().contiguous()
            assert idx.dim() == 1 and idx.dtype == torch.int32
            count, cap = None, idx.numel()
        if cap > 0:
            check(C.cbinfer_tail1x1(ptr(x), ptr(idx), cap, ptr(count), ptr(self._prepared()),
                                    ptr(self.bias1.detach()), ptr(self.weight2.detach().contiguous()),
                                    ptr(self.bias2.detach()), ptr(self.prevOutput), self.in_channels,
                                    self.hidden_channels, self.out_channels, H, W, int(self.relu),
                                    int(bool(self.withReLU)), stream_ptr(x)))
        if self.propChangeIndexes:
            return 'changeIndexes', self.prevOutput, indexes
        return self.prevOutput

    def __repr__(self):
        return '%s (%s->%s->%s, relu=%s, propChgIdxs=%s)' % (
            self.__class__.__name__, self.in_channels, self.hidden_channels, self.out_channels, self.relu,
            self.propChangeIndexes)
