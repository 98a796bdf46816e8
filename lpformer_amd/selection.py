"""Host side of the selection kernels: the per (stream, batch size) workspaces, how their buffers are sized, and the
status protocol of their control blocks (include/lpformer_hip.h, ``lpf_select_plan`` and ``lpf_select4``).  The launches
stay with the model (link_transformer.py: they read its thresholds, mask mode and graphs); a workspace takes them as
callables ``launch(ws, *args)``.

The protocol of all three forms: the kernels count what a batch needs even where the buffers are too small to hold it, so
the FIRST batch of a (stream, batch size) runs on token buffers, the counts are read back (synchronising) and the buffers
are sized from them (``calibrate``).  Later batches run without a read-back; one that does not fit raises STICKY bits in
``ctl`` (consumers clamp, its scores come out as NaN), and the next synchronising ``check`` clears them and marks the
workspace for sizing again."""
from __future__ import annotations

import collections

import torch

from . import _lib

# Words of a control block (int64; the header describes them under lpf_select_plan and lpf_select4).  Both generations
# keep the sticky bits and the totals per type in the same words, so the type-major consumers read either block.
CTL_ROOM = 0    # lpf_select4: entries the last batch needed room for (an upper bound); lpf_select(3)_plan: its slots
CTL_ITEMS = 1   # lpf_select(3)_plan: work items of the last batch; lpf_select4: its candidate slots (the true sum)
CTL_ERR = 3     # sticky LPF_SELECT_ERR_* bits: raised by the kernels, cleared by the host after handling
CTL_TOTALS = slice(4, 7)    # selected entries per type (cn, 1-hop, >1-hop): lpf_select(3)_run, lpf_select4_regions
assert CTL_TOTALS.stop <= min(_lib.CONST["LPF_SELECT_CTL_WORDS"], _lib.CONST["LPF_SELECT4_CTL_WORDS"])
Status = collections.namedtuple("Status", "err room items totals")

# ------------------------------------------------------------------------------------------ sizing policy
TOKEN = 16      # slots of a token buffer: the kernels drop what does not fit and still count it
_SLACK = 65536  # entries on top of a multiple of the first batch's, where the batches of one size differ most


def needs_resize(have: int, want: int, shrink: bool) -> bool:
    """The growth rule: allocate again when too small or -- ``shrink``: the exact sizing of a first batch -- more than
    twice too large (a workspace that met one hub-heavy batch does not keep that size forever)."""
    return want > have or (shrink and want < have // 2)


# Room from the counts of a first batch.  first_item_room / item_room: work items of a plan before / after anything is
# known about the batch; region_room: entries per TYPE REGION (one capacity for the three: twice the fullest);
# slot_room: pair-major entries -- a block's place is reserved for its candidate SLOTS (an upper bound of what it keeps):
# three times the first batch's, hub-heavy batches need several times the room of sparse ones; kept_room: selected
# entries the pair-major attention's scratch holds (its units of 16); blocks: blocks of LPF_SELECT4_BLOCK pairs.
def first_item_room(bs: int) -> int: return max(bs, 4096) + 16              # noqa: E704
def item_room(items: int) -> int: return 2 * items + 16                     # noqa: E704
def region_room(totals) -> int: return 2 * max(totals) + 4096               # noqa: E704
def slot_room(need: int) -> int: return 3 * need + _SLACK                   # noqa: E704
def kept_room(kept: int) -> int: return 2 * kept + _SLACK                   # noqa: E704
def blocks(bs: int) -> int: return -(-bs // _lib.SELECT4_BLOCK)             # noqa: E704


# ------------------------------------------------------------------------------------------ workspaces
class SelectionWorkspace:
    """What the forms share.  ``ctl`` persists across launches: its words are epoch-tagged or zero between launches, the
    host only ever clears the sticky one."""

    CTL_WORDS = _lib.CONST["LPF_SELECT4_CTL_WORDS"]

    def __init__(self, device, bs: int):
        self.device, self.bs = device, bs
        self.ctl = torch.zeros(self.CTL_WORDS, dtype=torch.int64, device=device)
        self.calibrated = False

    def _zeros(self, words: int) -> torch.Tensor:
        return torch.zeros(words, dtype=torch.int32, device=self.device)

    def _pair_major_tables(self):
        """What lpf_select4 leaves beside its entries: ``pair_tab`` int32 [bs, 4] = {first entry, n_cn, n_1hop,
        n_non1hop}, ``blk_cnt`` int32 [blocks + 1, 2] = {entries, pairs with entries} per block of pairs."""
        self.pair_tab = self._zeros(4 * max(self.bs, 1))
        self.blk_cnt = self._zeros(2 * blocks(self.bs) + 2)
        self.shape = 0          # launch shape of lpf_select4 (0 = the library's default)

    def _fit(self, name: str, cap: int, words: int, shrink: bool = False) -> int:
        """Buffer ``name`` with room for ``cap`` slots of ``words`` int32 each, under the growth rule; returns the
        capacity it has afterwards."""
        buf = getattr(self, name)
        have = 0 if buf is None else buf.numel() // words
        if not needs_resize(have, cap, shrink):
            return have
        setattr(self, name, None)  # release before allocating the new size
        setattr(self, name, self._zeros(int(cap) * words))
        return int(cap)

    def buffers(self):
        """Every device tensor the workspace owns right now: what a captured graph or a recorded plan keeps alive (a
        re-sized buffer is a new tensor)."""
        return [v for v in vars(self).values() if isinstance(v, torch.Tensor)]

    def read_status(self, stream=None) -> Status:
        """The control block by name.  The read is ordered after everything queued on ``stream`` (a
        ``torch.cuda.Stream``; default: the current one): the copy is issued ON that stream and waited for, so a
        selection kernel still in flight there cannot be read as "ok"."""
        with torch.cuda.stream(stream):     # (None: a no-op)
            v = self.ctl.tolist()
        return Status(int(v[CTL_ERR]), int(v[CTL_ROOM]), int(v[CTL_ITEMS]), [int(x) for x in v[CTL_TOTALS]])

    def clear_errors(self, stream=None):
        """Clears the sticky bits on ``stream`` (default: the current one) -- the stream whose kernels raise them, so
        the write cannot race with a kernel's atomicOr."""
        with torch.cuda.stream(stream):
            self.ctl[CTL_ERR] = 0

    def check(self, num_nodes: int, stream=None) -> Status:
        """Status read; where a batch since the last one did not fit: sticky bits cleared, node ids out of range raised
        as IndexError, else the workspace marked for sizing again."""
        s = self.read_status(stream)
        if s.err:
            self.clear_errors(stream)
            if s.err & _lib.SELECT_ERR_NODE_RANGE:
                raise IndexError(f"batch holds node ids outside [0, {num_nodes})")
            self.calibrated = False
        return s


class PlanRunWorkspace(SelectionWorkspace):
    """Type-major selection in two launches (lpf_select_plan / _run, lpf_select3_plan / _run): per type a region of
    ``ent_cap`` 16-byte records in ``entries``, int32 segment pointers in ``type_ptr``; ``desc`` / ``offs`` / ``item_pair``
    carry the plan, ``plan_lb`` / ``run_lb`` the chained-scan words (epoch-tagged, never cleared)."""

    CTL_WORDS = _lib.CONST["LPF_SELECT_CTL_WORDS"]

    def __init__(self, device, bs: int):
        super().__init__(device, bs)
        self.desc = torch.empty(16 * max(bs, 1), dtype=torch.int64, device=device)
        self.offs = torch.empty(bs + 1, dtype=torch.int64, device=device)
        self.plan_lb = torch.zeros(int(_lib.hip().lpf_select_plan_blocks(bs)) + 1, dtype=torch.int64, device=device)
        self.type_ptr = self._zeros(3 * (bs + 1))
        self.item_pair = self.run_lb = self.entries = None
        self.item_cap = self.ent_cap = 0

    def ensure(self, item_cap: int = 0, ent_cap: int = 0, shrink: bool = False):
        self.item_cap = self._fit("item_pair", item_cap, 1)     # (work items: never given back)
        self._fit("run_lb", item_cap, 3 * 2)                    # (three int64 scan words per item)
        self.ent_cap = self._fit("entries", ent_cap, 3 * 4, shrink)

    def calibrate(self, launch, *args, num_nodes: int):
        """One pass on token regions gives the totals; a batch of more work items than the first guess is planned
        again, three times at the most."""
        self.ensure(item_cap=first_item_room(self.bs), ent_cap=TOKEN)
        for _attempt in range(3):
            launch(self, *args)
            s = self.check(num_nodes)
            if not (s.err & _lib.SELECT_ERR_ITEM_CAP):
                break
            self.ensure(item_cap=item_room(s.items), ent_cap=TOKEN)
        else:
            raise _lib.LpfError("selection workspace could not be sized")
        self.ensure(item_cap=item_room(s.items), ent_cap=region_room(s.totals), shrink=True)
        self.calibrated = True


class PairMajorWorkspace(SelectionWorkspace):
    """The one-launch, pair-major selection (``lpf_select4``): ``ent_cap`` 16-byte records in ``entries``, a pair's run
    starts where its ``pair_tab`` entry says."""

    def __init__(self, device, bs: int):
        super().__init__(device, bs)
        self._pair_major_tables()
        self.entries = None
        self.ent_cap = 0
        self.kept_cap = 0       # selected entries the attention's scratch is sized for (its units of 16)

    pair_major = property(lambda self: (self.entries, self.ent_cap))     # lpf_select4's entry buffer and its capacity

    def ensure(self, ent_cap: int, shrink: bool = False):
        self.ent_cap = self._fit("entries", ent_cap, 4, shrink)

    def kept(self) -> int:
        """Selected entries of the last batch (synchronises)."""
        return int(self.blk_cnt[:-2:2].sum().item())

    def calibrate(self, launch, *args, num_nodes: int, shape):
        """The launch on a token buffer reports the room the batch needs and its candidate slots (``shape(bs, slots)``
        picks the launch shape from them); the sized launch then shows how many entries are kept."""
        self.ensure(ent_cap=TOKEN)
        launch(self, *args)
        s = self.check(num_nodes)
        self.shape = shape(self.bs, s.items)
        self.ensure(ent_cap=slot_room(s.room), shrink=True)
        launch(self, *args)
        self.kept_cap = kept_room(self.kept())
        self.calibrated = True


class RegionsWorkspace(SelectionWorkspace):
    """``lpf_select4`` + ``lpf_select4_regions``: the one-launch selection for consumers of the TYPE-MAJOR form (the
    matrix-core attention, the record-merging tail, ``lpf_select_export``).  To them it looks like a ``PlanRunWorkspace``
    (``type_ptr``, ``entries``, ``ent_cap``, ``ctl`` with the sticky bits and the totals per type); the pair-major half
    (``pair_tab``, ``blk_cnt``, ``blk_types``, ``entries4`` / ``ent_cap4``) stays inside."""

    def __init__(self, device, bs: int):
        super().__init__(device, bs)
        self._pair_major_tables()
        self.blk_types = self._zeros(4 * blocks(bs) + 4)     # {cn, 1-hop, >1-hop, 0} kept per block
        self.type_ptr = self._zeros(3 * (bs + 1))
        self.entries = self.entries4 = None
        self.ent_cap = self.ent_cap4 = 0

    pair_major = property(lambda self: (self.entries4, self.ent_cap4))

    def ensure(self, ent_cap: int, shrink: bool = False):
        self.ent_cap = self._fit("entries", ent_cap, 3 * 4, shrink)

    def calibrate(self, select4, regions, *args, num_nodes: int, shape):
        """``select4`` alone on a token buffer reports the room of the pair-major half (a block reserves its candidate
        slots there); ``regions`` -- both launches -- on token regions then gives the totals per type."""
        self.ent_cap4 = self._fit("entries4", TOKEN, 4)
        self.ensure(ent_cap=TOKEN)
        select4(self, *args)
        s = self.check(num_nodes)
        self.shape = shape(self.bs, s.items)
        self.ent_cap4 = self._fit("entries4", slot_room(s.room), 4, shrink=True)
        regions(self, *args)
        self.ensure(ent_cap=region_room(self.check(num_nodes).totals), shrink=True)
        self.calibrated = True
