"""The state of one running train / inference step, and the machinery that owns it: the zero-filled arena, the packed-weight
cache, the deferred weight-gradient work, the cached unit gradient, the side streams, and begin_step / end_step around them
(svnet_amd.train drives these).  What lives for one step and is replaced while it runs is an attribute of STEP, which is
itself never rebound: read `_step.STEP.<name>` at the time of use.  A leaf of the package: no op and no model is imported here.
"""
import torch


class _ZeroArena:
    """Zero-filled scratch of ONE training / inference step from a single fill: every accumulator of the step (BatchNorm sums,
    atomically accumulated gradients, ...) is a slice of one persistent buffer that `begin()` clears with one launch.  The slices
    are handed out in call order (a bump allocator), so a step that repeats asks for the same slices; what lies beyond the extent
    cleared at `begin()` (first step, a larger shape) falls back to torch.zeros and enlarges the extent for the next step.
    Slices stay valid until the next begin() - long enough for gradients, which the bucket copies before that.
    Every TrainStep / ForwardStep owns ITS arena (svnet_amd.train), and a step captured into a HIP graph pins it: the graph has
    the buffer's addresses baked in (the fill and every accumulator slice), so the buffer is never replaced afterwards and lives
    as long as the step object - another step, model or batch size cannot free or outgrow it under the graph's feet.
    Outside begin()/end() (tests calling single ops, ...) nothing is pooled."""

    def __init__(self):
        self.buf, self.zeroed, self.off, self.active, self.pinned = None, 0, 0, False, False

    def begin(self, dev, pin=False):
        need = (self.off + 4095) // 4096 * 4096
        if need and not self.pinned and (self.buf is None or self.buf.numel() < need or self.buf.device != torch.device(dev)):
            self.buf = torch.empty((need + need // 4 + (1 << 20),), dtype=torch.uint8, device=dev)
        self.zeroed = min(need, self.buf.numel()) if self.buf is not None else 0      # (pinned and outgrown: the rest comes from torch.zeros)
        if self.zeroed:
            self.buf[:self.zeroed].zero_()
        self.off, self.active = 0, True
        self.pinned = self.pinned or pin

    def end(self):
        self.active = False

    def take(self, nbytes, dev):
        if not self.active:
            return None
        o = self.off
        self.off += (nbytes + 255) // 256 * 256
        if self.buf is not None and self.off <= self.zeroed and self.buf.device == torch.device(dev):
            return self.buf[o:o + nbytes]
        return None


class _Step:
    """The records that live for one step.  begin_step installs the step's arena; the ops write the other three while the step
    runs; end_step puts all four back with restore()."""

    def __init__(self):
        self.default_arena = _ZeroArena()
        self.arena = self.default_arena      # the arena of the step that is running (begin_step / end_step)
        # Column sums a producer left for the BatchNorm over its output: (the [M, C] tensor itself - held, so that its memory cannot be
        # handed to another tensor while the record lives -, its version at the time, sums [2C] double).  Consumed once; any later
        # producer replaces it.
        self.fused_colsums = None
        self.sink = None                     # the _ops.CatSink whose `with` block is running
        self.knn_table = None                # (s.data_ptr(), v.data_ptr(), workspace, B, N, C) of the last prepared level (_ops.knn_table_ahead)

    def restore(self):
        self.knn_table = None                                 # (a prepared k-NN table nobody asked for is not held across steps)
        self.fused_colsums = None                             # (the producer's [M, O] output and its arena slice are not held across steps)
        self.sink = None
        self.arena.end()
        self.arena = self.default_arena


STEP = _Step()


def _zeros(shape, dtype, dev):
    n = 1
    for d in shape:
        n *= int(d)
    nbytes = n * torch.empty((), dtype=dtype).element_size()
    buf = STEP.arena.take(nbytes, dev) if nbytes else None
    if buf is None:
        return torch.zeros(tuple(shape), dtype=dtype, device=dev)
    return buf.view(dtype).view(tuple(shape))


def _zeros_pool(dev, *specs):
    """One zero-filled allocation (one fill launch, none inside a step: _ZeroArena) carved into tensors: specs are (shape, dtype) pairs."""
    offs, total = [], 0
    for shape, dtype in specs:
        n = 1
        for d in shape:
            n *= int(d)
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        offs.append((total, nbytes))
        total += (nbytes + 255) // 256 * 256
    buf = STEP.arena.take(max(total, 1), dev)
    if buf is None:
        buf = torch.zeros((max(total, 1),), dtype=torch.uint8, device=dev)
    return [buf[o:o + nb].view(dtype).view(shape) for (o, nb), (shape, dtype) in zip(offs, specs)]


_SIDE_STREAMS = {}


def _side_stream(dev):
    """One extra HIP stream per device for independent kernels of a fused backward (forked / joined with events, so the
    pattern is also valid inside a hipGraph capture)."""
    key = torch.device(dev).index if torch.device(dev).index is not None else torch.cuda.current_device()
    if key not in _SIDE_STREAMS:
        # (a high-priority side stream was measured: 10.7 ms per step against 6.4 - the tile kernel on the main stream starves)
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=key, priority=0)
    return _SIDE_STREAMS[key]


class _PlaneCache:
    """Packed forms of the binarized weights (sign / non-zero bit planes, +-1 values, scale*sign, the fused edge kernels' permuted
    planes and MFMA-fragment sign weights): sv_layers.py:44-48 re-derives sign(W) inside every forward; here a packed form is
    rebuilt only when its parameters CHANGED since it was packed - autograd's version counter (torch.optim steps, load_state_dict,
    in-place ops under no_grad) or the data address (re-homing into a flat buffer); writers that bypass both (the flat optimizer
    kernels of svnet_amd.train, anything going through .data or a raw pointer) call invalidate().  An eager step rebuilds the
    stale forms for all layers together on the side stream at its start (begin()), off the forward's critical path; a step
    replayed as a captured graph keeps the packing OUTSIDE the graph (begin(external=True) while capturing, refresh() before
    every replay).  Entries are created lazily the first time a layer asks (built inline that once).  Keys are the Parameter
    objects; the rebuild closures read their CURRENT data.  Outside begin()/end() every layer packs on the fly."""

    def __init__(self):
        self.entries, self.active, self.event, self.waited = {}, False, None, None      # waited: ids of the streams that have joined
        self.sig, self.dirty = {}, False        # (version counter, address) of every entry's parameters at its last (re)build

    @staticmethod
    def _signature(params):
        return tuple((p._version, p.data_ptr()) for p in params)

    def invalidate(self):
        """The weights were changed behind autograd's back (a raw kernel on a flat parameter buffer: svnet_amd.train's optimizers call
        this; so must anything else that writes through .data or a raw pointer): rebuild everything at the next step."""
        self.dirty = True

    def _stale(self):
        """Entries whose parameters changed since they were packed (autograd version counter or address), or all after invalidate()."""
        out = []
        for key in list(self.entries):
            refs, _, rebuild = self.entries[key]
            ps = [r() for r in refs]
            if any(p is None for p in ps):
                del self.entries[key]                 # the parameters are gone (another model was built)
                self.sig.pop(key, None)
            elif self.dirty or self.sig.get(key) != self._signature(ps):
                out.append((key, ps, rebuild))
        return out

    def refresh(self, dev):
        """Re-pack what is stale, on the CURRENT stream.  For a step that is replayed as a captured graph (the packing launches are
        not part of the graph: they depend on whether an optimizer ran in between) - svnet_amd.train calls it before every replay."""
        for key, ps, rebuild in self._stale():
            rebuild()
            self.sig[key] = self._signature(ps)
        self.dirty = False

    def rebuild_all(self, run=None):
        """Every live entry re-packed now, whatever its state (run(rebuild) issues one; default: on the current stream) - what a
        captured optimizer step records behind its update kernel (svnet_amd.train).  Returns the entries' keys."""
        keys = []
        for key in list(self.entries):
            refs, _, rebuild = self.entries[key]
            if any(r() is None for r in refs):
                continue
            (run or (lambda f: f()))(rebuild)
            keys.append(key)
        return keys

    def mark_fresh(self, keys):
        """The given entries have just been re-packed from the parameters' current values by someone else (a replayed graph)."""
        for key in keys:
            e = self.entries.get(key)
            if e is not None:
                ps = [r() for r in e[0]]
                if all(p is not None for p in ps):
                    self.sig[key] = self._signature(ps)

    def _join(self):
        if self.waited is not None:
            st = torch.cuda.current_stream()
            if st.cuda_stream not in self.waited:
                st.wait_event(self.event)
                self.waited.add(st.cuda_stream)

    def begin(self, dev, external=False):
        """external: the step is being captured into a graph - its packed forms are kept fresh by refresh() before every replay."""
        self.active, self.waited = True, None
        if external:
            return
        stale = self._stale()
        if stale:
            main, side = torch.cuda.current_stream(dev), _side_stream(dev)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                for key, ps, rebuild in stale:
                    rebuild()
                    self.sig[key] = self._signature(ps)
                self.event = side.record_event()
            self.waited = {side.cuda_stream}
        self.dirty = False

    def end(self):
        if self.active:                          # (also when nothing looked anything up: graph capture needs the side stream joined)
            self._join()
        self.active = False

    def get(self, kind, params, build):
        """build() -> (outputs, rebuild): packs now; rebuild() re-packs into the same output tensors."""
        if not self.active:
            return build()[0]
        key = (kind,) + tuple(id(p) for p in params)
        e = self.entries.get(key)
        if e is not None and all(r() is p for r, p in zip(e[0], params)):
            self._join()
            return e[1]
        import weakref
        out, rebuild = build()
        self.entries[key] = (tuple(weakref.ref(p) for p in params), out, rebuild)
        self.sig[key] = self._signature(params)
        return out


PLANES = _PlaneCache()


class _Deferred:
    """Weight-gradient work that nothing in the backward pass waits for (svnet_amd.train.TrainStep only: it gathers the parameter
    gradients ONCE, after the backward).  While `active`, a fused edge layer's backward leaves its weight-gradient chain (linear1's
    product, linear2's, the parameter epilogue) on the side stream WITHOUT joining it into the main stream, which goes on with the next
    layer's backward; `join()` (called before the gradients are packed) is the one join.  `keep` holds every tensor those kernels
    touch until then: the caching allocator would otherwise hand their blocks - freed when the backward function returns - to the
    main stream's next allocation while the side stream still reads them.  Off (plain autograd use of the layers): every backward
    joins before it returns, as before."""

    def __init__(self):
        self.active = False
        self.keep = []
        self.seen = set()

    def first_use(self, *params):
        """True while none of `params` (a layer's weights) has been handed an unwritten gradient in this backward.  A module applied
        twice in one forward - or one parameter read by two Functions - gets two gradients, which autograd ADDS on the main stream:
        the second backward must therefore take the joined schedule (its final join also covers the first, deferred chain).  This is
        the run-time half of TrainStep._deferral_is_safe(), which can only see parameters registered under two names."""
        keys = [p.data_ptr() for p in params if p is not None]
        dup = any(k in self.seen for k in keys)
        self.seen.update(keys)
        return not dup

    def join(self, dev):
        if self.keep:
            torch.cuda.current_stream(dev).wait_stream(_side_stream(dev))
            self.keep.clear()
        self.seen.clear()


DEFERRED = _Deferred()


class _UnitGrad:
    """One cached scalar 1.0 per device: a train step seeds its backward with it (`torch.autograd.backward(loss, UNIT_GRAD.get(dev))`)
    instead of `loss.backward()`'s fresh ones_like, and SmoothCE.backward recognises it BY IDENTITY - the fill kernel and the
    multiplication by one were two launches (~10 us) on the critical path between the forward and the backward."""

    def __init__(self):
        self.t = {}

    def get(self, dev):
        dev = torch.device(dev)
        key = (dev.type, dev.index if dev.index is not None else (torch.cuda.current_device() if dev.type == "cuda" else 0))
        if key not in self.t:
            self.t[key] = torch.ones((), dtype=torch.float32, device=dev)
        return self.t[key]


UNIT_GRAD = _UnitGrad()


def begin_step(dev, planes_external=False, arena=None):
    """Start of a train / inference step (svnet_amd.train): one fill for the step's zero-initialised scratch (`arena`: the step
    object's own _ZeroArena; `planes_external` = the step is being captured into a HIP graph, which also pins the arena), and the
    packed weight forms of the layers whose weights changed since they were last packed rebuilt on the side stream."""
    STEP.arena = arena if arena is not None else STEP.default_arena
    STEP.arena.begin(dev, pin=planes_external)
    PLANES.begin(dev, planes_external)


def end_step():
    STEP.restore()
    PLANES.end()
    DEFERRED.active = False
    DEFERRED.keep.clear()
    DEFERRED.seen.clear()
