"""The one liveness rule of everything the engine caches per parameter: the packed weight copies of the inference path
(hip._PackedWeights) and of the training step (archs/nhwc_train._PackTable), and the fp16 weight scales (nhwc_train._WeightScales)."""
import collections
import weakref

ParamStamp = collections.namedtuple('ParamStamp', 'alive ptr version epoch')


def param_stamp(weight, epoch=None):
    """What a cache entry made from ``weight`` (the parameter, or None where the entry's weak reference has died) remembers of it:
    the copy is good while ``param_stamp(entry.ref(), ...) == entry.stamp``.  The stamp moves when the parameter is modified in a
    way autograd sees (optimiser step, load_state_dict, an in-place op under no_grad: ``_version``) or its storage is replaced
    (``p.data = ...``, ``.to()``: ``data_ptr``); it reads dead once the parameter is gone; a write THROUGH ``p.data`` moves nothing.
    ``epoch``: hip.capture_epoch()[1], for copies that are not replayed with a graph captured on the other side of a boundary."""
    return ParamStamp(False, 0, -1, epoch) if weight is None else ParamStamp(True, weight.data_ptr(), weight._version, epoch)


class Packed:
    """a packed copy: the parameter (weak), the copy, the parameter's stamp when the copy was made; in the training tables also
    the job that refills it and the refresh that last saw it asked for"""
    __slots__ = ('ref', 'packed', 'stamp', 'job', 'last_used')

    def __init__(self, weight, packed, stamp, job=None, last_used=0):
        self.ref, self.packed, self.stamp, self.job, self.last_used = weakref.ref(weight), packed, stamp, job, last_used
