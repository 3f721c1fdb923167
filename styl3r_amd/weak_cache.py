"""One cache for things derived from a tensor (vit_ops: split weight images, weight |max| words, derived weights, published |max| words).

The validity rule, in one place: a cached payload is valid while the SAME TENSOR OBJECT it was derived from is alive, still starts at
the SAME ADDRESS and carries the VERSION it was stored with.
  * weak reference, not the id or the address alone: a new tensor that happens to reuse a dead one's id / address never hits the entry, and
    the callback drops the entry (and the device buffer it holds) the moment the tensor dies -- per-step temporaries (the reshaped
    ConvTranspose / strided-conv weights of the DPT reassemble stage) must not pile up.
  * address: `p.data = other` keeps the object and its version counter but moves it to other memory (ddp.BucketedGradReducer in "rs_ag"
    mode re-homes every parameter in a flat buffer this way); a payload that holds addresses or was built from the old bytes is stale.
  * version: `load_state_dict` and in-place torch ops bump `Tensor._version`; optimizer steps do NOT by themselves (optim.AdamWHIP writes
    through raw pointers, and the framework's fused AdamW leaves the counter alone, too), so AdamWHIP.step and train.make_optimizer's
    post-step hook bump it explicitly (without that the kernels kept computing with the first split of every weight).  Writes
    through `weight.data` bypass the counter -- vit_ops.invalidate_split_cache() after such surgery.
Host cost: a lookup is one dictionary access plus field compares and allocates nothing; nothing here iterates over the dictionary (the
weak-reference callbacks fire at any time, also on the autograd engine thread).
"""
from weakref import ref


class Entry(ref):
    """the weak reference to the owner tensor itself -- `entry()` is the owner or None -- with the key, the version and address it was stored at,
    the payload and (vit_ops._PUBLISHED) the raw stream as named fields"""
    __slots__ = ("key", "version", "ptr", "payload", "stream")


class WeakTensorCache:
    """key -> Entry"""
    __slots__ = ("_entries", "entry")

    def __init__(self):
        self._entries: dict = {}
        self.entry = self._entries.get      # entry(key): the raw Entry or None, for callers with a lookup rule of their own (vit_ops._known_amax, refresh_split_cache)

    def _drop(self, dead: Entry) -> None:
        """the one weak-reference callback: the entry goes with its owner -- unless a newer owner has taken the key since"""
        if self._entries.get(dead.key) is dead:
            del self._entries[dead.key]

    def get(self, key, owner):
        """the payload stored under `key`, if it is still valid for `owner` (the rule above); else None"""
        e = self._entries.get(key)
        return e.payload if (e is not None and e() is owner and e.version == owner._version and e.ptr == owner.data_ptr()) else None

    def previous(self, key, owner):
        """the payload last stored under `key` for the same live `owner`, whatever its version (a stale image's buffer is reused); else None"""
        e = self._entries.get(key)
        return e.payload if e is not None and e() is owner else None

    def store(self, key, owner, payload, stream: int = 0) -> None:
        e = Entry(owner, self._drop)
        e.key, e.version, e.ptr, e.payload, e.stream = key, owner._version, owner.data_ptr(), payload, stream
        self._entries[key] = e

    def renew(self, key, owner) -> None:
        """the payload under `key` was rebuilt in place from `owner`'s present values: current again at its present version"""
        e = self._entries[key]
        e.version, e.ptr = owner._version, owner.data_ptr()

    def __len__(self) -> int:
        return len(self._entries)

    def __contains__(self, key) -> bool:
        return key in self._entries

    def clear(self) -> None:
        self._entries.clear()
