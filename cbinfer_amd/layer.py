"""What the weight-carrying layers that run their own change detection share on the host:
CBDetectingLayer, the base of CBDepthwiseConv2d, CBGroupedConv2d and CBConvTranspose2d -- constructor, state
(prevInput / prevOutput), geometry struct, frame-mask workspace, operand intake and the prevInput hand-over -- and
CBContractingLayer, which adds the arithmetic choice and the prepared-weights cache of the two MFMA layers.  A subclass
file keeps its limits and its `_check_*`, its C call, its `__repr__` and its link or insert pass.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from ._lib import C, CBinferError, dtype_code, require_device
from .chain import state_fits
from .conv2d import _switch


def check_limits(name, limits, axes=(0, 1)):
    """CBinferError for the first axis, and on it the first (setting name, pair, limit) of `limits`, beyond a limit."""
    for i in axes:
        for setting, pair, limit in limits:
            if pair[i] > limit:
                raise CBinferError("%s: %s=%s is beyond what the library takes (<= %d per axis)"
                                   % (name, setting, pair, limit))


def frame_masks(Ho, Wo, dev):
    """(frame masks of the layer's own detection on an Ho x Wo output map, zero once; their mask-copy view)."""
    bits = torch.zeros(C.cbinfer_frame_mask_bytes(Ho, Wo) // 8, dtype=torch.int64, device=dev)
    off = C.cbinfer_frame_mask_copy_offset(Ho, Wo) // 8
    return bits, bits[off:off + C.cbinfer_mask_words(Ho, Wo)]


class CBDetectingLayer(nn.Module):
    """A change-based layer with parameters, batch 1, that keeps prevInput and prevOutput.  A subclass passes what its
    `_check_*` returned -- one pair per name of _GEOM_FIELDS -- and, where it is no plain cbGeom layer, names its
    geometry struct and output-size function and writes `_no_output`, the sentence for a map without output."""
    _TRANSIENT = ('_work', '_geomC')      # made again on demand: device work buffers, ctypes arguments
    _GEOM = _lib.Geom
    _GEOM_FIELDS = ('kernel_size', 'stride', 'padding', 'dilation')
    _OUT_SIZE = C.cbinfer_geom_out_size

    def __init__(self, m, threshold, geometry):
        super(CBDetectingLayer, self).__init__()
        for name, pair in zip(self._GEOM_FIELDS, geometry):
            setattr(self, name, pair)
        self.groups = m.groups
        self.transposed = False
        self.in_channels = m.in_channels
        self.out_channels = m.out_channels
        self.weight = m.weight      # shared with the source module
        self.bias = m.bias
        self.threshold = threshold
        self.withReLU = False
        self.propChangeIndexes = False
        self.copyInput = True
        self.feedbackLoop = False
        self.cloneOutput = True
        self.clearMemory()

    # ---------------------------------------------------------------- state
    def clearMemory(self):
        for name in ('prevInput', 'prevOutput'):
            if name not in self._buffers:
                self.register_buffer(name, self.weight.detach().new_zeros(0))
        self.prevInput = self.weight.detach().new_zeros(0)
        self.prevOutput = self.weight.detach().new_zeros(0)
        for name in self._TRANSIENT:
            self.__dict__[name] = None

    def getStateTensors(self):
        return [self.prevInput, self.prevOutput]

    def __getstate__(self):
        d = dict(self.__dict__)
        d.update(dict.fromkeys(self._TRANSIENT))
        return d

    def _struct(self):
        """(pointer to) the layer's cbGeom / cbTGeom; transient, made again after unpickling."""
        if self.__dict__.get('_geomC') is None:
            self.__dict__['_geomC'] = ctypes.pointer(self._GEOM(*(v for name in self._GEOM_FIELDS
                                                                  for v in getattr(self, name))))
        return self.__dict__['_geomC']

    def _out_hw(self, Hi, Wi):
        Ho, Wo = ctypes.c_int(), ctypes.c_int()
        if self._OUT_SIZE(Hi, Wi, self._struct(), ctypes.byref(Ho), ctypes.byref(Wo)) != 0:
            raise CBinferError(self._no_output(Hi, Wi))
        return Ho.value, Wo.value

    def _no_output(self, Hi, Wi):
        return ("%s: a %dx%d map is smaller than the filter's reach (kernel_size=%s, dilation=%s, padding=%s)"
                % (type(self).__name__, Hi, Wi, self.kernel_size, self.dilation, self.padding))

    def _act(self):
        return _lib.ACT_RELU if self.withReLU else _lib.ACT_NONE

    def _bias_map(self, size, like):
        """The dense value of an output pixel no tap reaches, broadcast over the map: the bias (0 without one), after
        the activation.  The first frame overwrites every reachable pixel."""
        fill = torch.zeros(size, dtype=like.dtype, device=like.device)
        if self.bias is not None:
            b = self.bias.detach().to(device=like.device, dtype=like.dtype)
            act = self._act()
            if act != _lib.ACT_NONE:
                b = torch.relu(b) if act == _lib.ACT_RELU else torch.clamp(b, 0.0, 6.0)
            fill += b.view(1, -1, 1, 1)
        return fill

    def _state_for(self, input, Ho, Wo, keepInput=True):
        """(Re)allocate the state on a new resolution, dtype or device: prevInput +inf -- the first frame of a sequence
        is dense through the same kernels, every input pixel changed --, contiguous if it was kept, and dropped without
        keepInput.  True if prevOutput was (re)allocated."""
        if not keepInput:
            if self.prevInput.numel():
                self.prevInput = input.new_zeros(0)
        elif not state_fits(self.prevInput, input.size(), input):
            self.prevInput = torch.full(input.size(), float('inf'), dtype=input.dtype, device=input.device)
        elif not self.prevInput.is_contiguous():
            self.prevInput = self.prevInput.contiguous()
        size = (1, self.out_channels, Ho, Wo)
        if not state_fits(self.prevOutput, size, input):
            self.prevOutput = self._bias_map(size, input)
            return True
        return False

    def _buffers_for(self, Ho, Wo, dev):
        """Frame masks `bits` and their mask-copy view `copy`, index buffer and count for a consumer that wants the
        list."""
        bits, copy = frame_masks(Ho, Wo, dev)
        return dict(bits=bits, copy=copy, idx=torch.empty(Ho * Wo, dtype=torch.int32, device=dev),
                    count=torch.zeros(1, dtype=torch.int32, device=dev))

    def _workspace(self, Hi, Wi, dev):
        """The layer's work buffers and the `size` of its output map: once per map size."""
        key = (Hi, Wi, dev)
        work = self.__dict__.get('_work')
        if work is None or work['key'] != key:
            Ho, Wo = self._out_hw(Hi, Wi)
            work = self.__dict__['_work'] = dict(self._buffers_for(Ho, Wo, dev), key=key, size=(Ho, Wo))
        return work

    # ---------------------------------------------------------------- frame
    def _operand(self, inp):
        """(contiguous [1, C, Hi, Wi] tensor on the weights' device, change indexes or None, whether the tensor is a
        producer's live in-place state) of forward's argument."""
        indexes = None
        if type(inp) == tuple:
            if len(inp) != 3 or inp[0] != 'changeIndexes':
                raise CBinferError("%s: the input is a tuple, but not ('changeIndexes', tensor, indexes)"
                                   % type(self).__name__)
            inp, indexes = inp[1], inp[2]
        if not torch.is_tensor(inp):
            raise CBinferError("%s: the input must be a tensor or the ('changeIndexes', tensor, indexes) tuple, got %s"
                               % (type(self).__name__, type(inp).__name__))
        live = bool(getattr(inp, '_cbinfer_inplace_state', False))
        x = inp.detach().contiguous()
        if x.dim() != 4 or x.size(0) != 1 or x.size(1) != self.in_channels:
            raise CBinferError("%s: the input must be a [1, %d, H, W] tensor, got %s"
                               % (type(self).__name__, self.in_channels, tuple(x.shape)))
        require_device(x)
        if x.dtype != self.weight.dtype or x.device != self.weight.device:
            raise CBinferError("%s: input (%s on %s) and weights (%s on %s) differ in dtype or device"
                               % (type(self).__name__, x.dtype, x.device, self.weight.dtype, self.weight.device))
        return x, indexes, live

    def _keep_input(self, x, live):
        """After the frame's call: without feedback and without a copy by the kernel, the frame itself is prevInput -- a
        producer's live in-place state as a clone, since the producer writes it again."""
        if not self.feedbackLoop and not self.copyInput:
            self.prevInput = x.clone() if live else x


class CBContractingLayer(CBDetectingLayer):
    """A CBDetectingLayer whose contraction runs on the MFMA units: exactF32 and the arithmetic it selects, and the
    weights in the kernels' layout, prepared once per weights, map size and arithmetic.  A subclass writes
    `_prepare(w, Hi, Wi, arith)`: the prepared form of the contiguous weights `w`, made by its own two C entry points
    (every launching call of a layer is made in its own module, through that module's `C`)."""
    _TRANSIENT = ('_work', '_wprep', '_geomC')

    def __init__(self, m, threshold, geometry):
        super(CBContractingLayer, self).__init__(m, threshold, geometry)
        self.exactF32 = False

    def invalidateWeights(self):
        """Forget the cached prepared weights -- after a write through `weight.data`, which bumps neither the Parameter
        object nor its version counter."""
        self.__dict__['_wprep'] = None

    def _arith(self, t):
        if dtype_code(t) == _lib.CB_F16:
            return _lib.CB_F16
        return _lib.CB_F32 if (self.exactF32 or _switch('CBINFER_EXACT_F32')) else _lib.CB_F32S

    def _weights(self, Hi, Wi, arith):
        w = self.weight
        key = (w.data_ptr(), w._version, w.dtype, w.device, Hi, Wi, arith)
        wprep = self.__dict__.get('_wprep')
        if wprep is None or wprep[0] != key:
            wprep = self.__dict__['_wprep'] = (key, self._prepare(w.detach().contiguous(), Hi, Wi, arith))
        return wprep[1]
