"""Without a GPU: tests/poison.py's poisoned_empty really fills what the wrapped allocators hand out and puts the originals back; and a
reading of csrc/f3d_ctx.h and f3d_debug_poison (csrc/f3d_ctx.cpp) -- every device pointer member of the context and every scratch and
kept slot has a decision in POLICY below ('poisoned' or 'left: <reason>', the rows of DESIGN 2.2), and the hook's source does what
the decision says.  A slot or member added without deciding fails here."""
import re

import numpy as np
import pytest

import f3d
from conftest import ROOT, PKG
from poison import poisoned_empty

CSRC = PKG / 'csrc'
PATTERNS = [0x00, 0xFF, 0x5A]
NP_DTYPES = [np.bool_, np.uint8, np.int8, np.uint16, np.int16, np.int32, np.uint32, np.int64, np.uint64, np.float16, np.float32, np.float64]


def all_bytes(a, byte):
    raw = a.tobytes()                                       # every element's bytes, whatever the order
    return raw == bytes([byte]) * len(raw)


# ---- a. poisoned_empty ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('byte', PATTERNS)
def test_numpy_allocations_hold_the_pattern(byte):
    with poisoned_empty(byte):
        for dt in NP_DTYPES:
            for a in (np.empty(7, dt), np.empty((3, 5), dtype=dt), np.empty((3, 5), dt, order='F'), np.empty((), dt), np.empty(0, dt),
                      np.empty((4, 0, 2), dt), np.empty_like(np.zeros((2, 3), dt)), np.empty_like(np.zeros((2, 3), dt), order='F'),
                      np.empty_like(np.zeros((5, 4, 3), np.int8), dtype=dt), np.empty_like(np.zeros((4, 6), dt).T),
                      np.empty_like(np.zeros((2, 3, 4), dt).transpose(1, 0, 2)), np.empty_like(np.zeros(9, np.float32), shape=(2, 2), dtype=dt)):
                assert a.dtype == np.dtype(dt) and a.flags.writeable
                assert all_bytes(a, byte), (dt, a.shape)
        assert np.empty((3, 5), np.float64, order='F').flags.f_contiguous and np.empty_like(np.zeros((4, 6)).T).flags.f_contiguous
        assert np.empty(2, object)[0] is None                                   # object arrays are left alone
    if byte == 0xFF:
        with poisoned_empty(byte):
            assert np.isnan(np.empty(3)).all() and (np.empty(3, np.int32) == -1).all() and np.isnan(np.empty(3, np.float16)).all()
            assert (np.empty(3, np.uint16) == 0xFFFF).all()
    if byte == 0x5A:
        with poisoned_empty(byte):
            x = np.empty(3)
            assert np.isfinite(x).all() and (x > 1e100).all() and (np.empty(3, np.int64) == 0x5A5A5A5A5A5A5A5A).all()


@pytest.mark.parametrize('byte', PATTERNS)
def test_torch_allocations_hold_the_pattern(byte):
    import torch
    dtypes = [torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.float16, torch.bfloat16, torch.float32, torch.float64]
    if hasattr(torch, 'uint16'):
        dtypes.append(torch.uint16)
    with poisoned_empty(byte):
        for dt in dtypes:
            base = torch.zeros((3, 4), dtype=dt)
            for t in (torch.empty(7, dtype=dt), torch.empty((3, 5), dtype=dt), torch.empty(3, 5, dtype=dt, device='cpu'), torch.empty((), dtype=dt),
                      torch.empty(0, dtype=dt), torch.empty((2, 0, 3), dtype=dt), torch.empty_like(base), torch.empty_like(base.t()),
                      torch.empty_like(base, dtype=torch.int16), base.new_empty(5), base.new_empty((2, 3)),
                      base.new_empty((2, 2), dtype=torch.float64), base.new_empty(0),
                      torch.empty((2, 3, 4, 5), dtype=dt, memory_format=torch.channels_last)):
                raw = torch.tensor([], dtype=torch.uint8).set_(t.untyped_storage()) if t.numel() else torch.tensor([], dtype=torch.uint8)
                assert raw.numel() == t.numel() * t.element_size() and bool((raw == byte).all()), (dt, tuple(t.shape))
        assert torch.empty(7).dtype == torch.get_default_dtype()
        assert torch.empty_like(base.t()).stride() == base.t().stride()
        o = torch.zeros(2)
        assert torch.empty(4, out=o) is o and o.shape == (4,)                   # out=: the caller's tensor, passed through


def test_the_originals_are_back_after_the_block_and_after_an_exception():
    import torch
    before = (np.empty, np.empty_like, torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with poisoned_empty(0x5A):
        assert all(a is not b for a, b in zip(before, (np.empty, np.empty_like, torch.empty, torch.empty_like, torch.Tensor.new_empty)))
    assert before == (np.empty, np.empty_like, torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with pytest.raises(KeyError):
        with poisoned_empty(0xFF):
            raise KeyError('inside')
    assert before == (np.empty, np.empty_like, torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with poisoned_empty(1):                                                     # nested blocks unwind in order
        with poisoned_empty(2):
            assert np.empty(2, np.uint8).tolist() == [2, 2]
        assert np.empty(2, np.uint8).tolist() == [1, 1]
    assert before == (np.empty, np.empty_like, torch.empty, torch.empty_like, torch.Tensor.new_empty)
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            with poisoned_empty(bad):
                pass
    assert before == (np.empty, np.empty_like, torch.empty, torch.empty_like, torch.Tensor.new_empty)


def test_the_product_does_not_import_the_poisoner():
    for p in list(PKG.rglob('*.py')) + [ROOT / 'bench.py', ROOT / '__graft_entry__.py']:
        assert not re.search(r'^\s*(from|import)\s+(tests\.)?(poison|family_cases)\b', p.read_text(), re.M), p


def test_the_product_spells_its_allocations_as_module_attributes():
    """poisoned_empty replaces module attributes; an `empty` bound by name at import time would slip past it."""
    for p in PKG.rglob('*.py'):
        assert not re.search(r'^\s*from\s+(numpy|torch)\s+import\s+[^\n]*\bempty', p.read_text(), re.M), p


# ---- b. the policy ------------------------------------------------------------------------------------------------------------------
POISONED = 'poisoned'
SCRATCH_SLOTS = ['SLOT_OBB_BOXES', 'SLOT_SORT_PERM', 'SLOT_SORT_SCRATCH', 'SLOT_TILED_MASKS', 'SLOT_TODO', 'SLOT_GRAPH', 'SLOT_GRAPH_BBOX',
                 'SLOT_PATCH', 'SLOT_GRP_SCRATCH', 'SLOT_OBB_TABLE', 'SLOT_OBB_FACETS', 'SLOT_OBB_CAND', 'SLOT_FUSE_TABLES', 'SLOT_FUSE_CARRY',
                 'SLOT_FUSE_XYZ', 'SLOT_FUSION', 'SLOT_PATCH_STATUS', 'SLOT_NRM', 'SLOT_NRM_CAMS', 'SLOT_QRY', 'SLOT_FLOOD', 'SLOT_COLOR',
                 'SLOT_CVS_INST', 'SLOT_CVS_STATS', 'SLOT_QUADS', 'SLOT_GROW', 'SLOT_PVOTE', 'SLOT_PVOTE_BITS', 'SLOT_MESH', 'SLOT_ZKEY',
                 'SLOT_ZCOUNTS', 'SLOT_KNN', 'SLOT_KNN_FLAG', 'SLOT_PLANES', 'SLOT_RASTER', 'SLOT_ZLUT', 'SLOT_SMOOTH', 'SLOT_FACE_GRAPH',
                 'SLOT_LIFT', 'SLOT_LIFT_TABLE', 'SLOT_TSDF', 'SLOT_ICP']
KEPT_SLOTS = ['KEPT_GRAPH_OFFS', 'KEPT_QRY_IN', 'KEPT_QRY_OFFS', 'KEPT_GRP_ORDER', 'KEPT_GRP_KEYS', 'KEPT_GRP_STARTS', 'KEPT_GRP_XYZ', 'KEPT_TSDF']
POLICY = {
    **{s: POISONED for s in SCRATCH_SLOTS},                 # the whole scratch[] array, over each buffer's capacity
    **{k: POISONED for k in KEPT_SLOTS},                    # the whole kept[] array; the sequences that own them are ended
    'stage': POISONED,                                      # the whole stage[] array: nothing in it outlives a call
    'scratch': POISONED,
    'kept': POISONED,
    'filter_dev': POISONED,                                 # make_filter uploads the list of every call that has one
    'count_dev': POISONED,                                  # f3d_relabel clears it before the launch
    'first_bad': POISONED,                                  # set to "no bad frame" at the head of every batched vote
    'pv_words': POISONED,                                   # the point vote's pre-pass sets all four words
    'table': POISONED,                                      # and table_stamped = false: the next batched vote clears the set
    'dev_err': 'left: the sticky device error word holds the bits of operations whose error nobody has taken yet',
    'codebook': 'left: its presence set is kept zero between calls (whoever sets bits clears them); zeroed once at creation',
    'stream': 'left: a stream handle, not device memory',
    'qry_queries': 'left: the caller\'s query pointer of the last count pass, compared and never read through; qry_n = -1 ends the sequence',
    'chunk.perm': 'left: the caller\'s pointers of a view-chunked fused call; the hook is refused while one is active',
    'chunk.xyz': 'left: the caller\'s pointers of a view-chunked fused call; the hook is refused while one is active',
}
ENDED = ['graph_n = -1', 'graph_kept = false', 'qry_n = -1', 'qry_kept = false', 'grp_n = -1', 'grp_cloud = false', 'tsdf_n = -1',
         'tsdf_kept = false', 'table_stamped = false']


def _braces(text, at):
    i = text.index('{', at)
    depth = 0
    for j in range(i, len(text)):
        depth += text[j] == '{'
        depth -= text[j] == '}'
        if depth == 0:
            return text[i + 1:j]
    raise AssertionError('unbalanced braces')


def context_header():
    text = (CSRC / 'f3d_ctx.h').read_text()
    text = re.sub(r'//[^\n]*', '', text)
    slots = [s.strip() for s in re.sub(r'=\s*0', '', _braces(text, text.index('enum scratch_slot'))).split(',')]
    kept = [s.strip() for s in re.sub(r'=\s*0', '', _braces(text, text.index('enum kept_slot'))).split(',')]
    body = _braces(text, text.index('struct f3d_ctx {'))
    members = []
    inner = re.search(r'struct\s*\{([^{}]*)\}\s*(\w+)\s*;', body)                # the one nested struct: chunk
    if inner:
        members += [f'{inner.group(2)}.{m}' for m in re.findall(r'\*\s*(\w+)\s*[;,]', inner.group(1))]
        body = body.replace(inner.group(0), '')
    members += re.findall(r'\*\s*(\w+)\s*;', body)                               # `type* name;`
    members += re.findall(r'\bhipStream_t\s+(\w+)\s*;', body)
    arrays = re.findall(r'\bdevbuf\s+(\w+)\s*\[', body)
    return slots, kept, members, arrays


def hook_source():
    text = (CSRC / 'f3d_ctx.cpp').read_text()
    return _braces(text, text.index('int f3d_debug_poison('))


def test_the_header_is_read_as_expected():
    slots, kept, members, arrays = context_header()
    assert slots[-1] == 'SLOT_COUNT' and kept[-1] == 'KEPT_COUNT' and len(slots) == 43 and len(kept) == 9
    assert sorted(arrays) == ['kept', 'scratch', 'stage']
    assert {'dev_err', 'table', 'first_bad', 'filter_dev', 'count_dev', 'codebook', 'pv_words', 'stream', 'qry_queries'} <= set(members)


def test_every_slot_and_every_pointer_member_has_a_policy():
    slots, kept, members, arrays = context_header()
    declared = slots[:-1] + kept[:-1] + members + arrays
    assert len(declared) == len(set(declared))
    assert sorted(declared) == sorted(POLICY)                                    # none undecided, none stale
    for key, what in POLICY.items():
        assert what == POISONED or re.fullmatch(r'left: \S.{20,}', what), key


def test_the_hook_treats_every_key_as_the_policy_says():
    src = hook_source()
    slots, kept, members, arrays = context_header()
    for a in arrays:                                                             # the three arenas: every buffer, its whole capacity
        assert POLICY[a] == POISONED and re.search(r'for \(devbuf& b : ctx->' + a + r'\) F3D_HIP\(ctx, fill\(b\.p, b\.cap\)\);', src), a
    assert all(POLICY[s] == POISONED for s in slots[:-1] + kept[:-1])            # ... so no slot of theirs can be 'left'
    for m in members:
        filled = re.search(r'fill\(ctx->' + re.escape(m) + r'\b', src) is not None
        assert filled == (POLICY[m] == POISONED), m
        if not filled:
            assert not re.search(r'ctx->' + re.escape(m) + r'\b(?!,)', src.replace('ctx->stream)', '')), m    # left means untouched
    for line in ENDED:
        assert f'ctx->{line};' in src, line
    assert 'ctx->chunk.active' in src and 'byte < 0 || byte > 255' in src
    assert src.count('hipStreamSynchronize(ctx->stream)') == 2 and 'getenv' not in (CSRC / 'f3d_ctx.cpp').read_text()
    assert src.index('hipStreamSynchronize') < src.index('fill(b.p') < src.rindex('hipStreamSynchronize')


def test_no_other_entry_looks_at_the_hook():
    """It adds nothing to any other entry's path: the one library source that names it is the one that defines it."""
    hits = [(p.name, n) for p in CSRC.iterdir() if p.suffix in ('.cpp', '.hip', '.h') for n in [p.read_text().count('debug_poison')] if n]
    assert [name for name, _ in hits] == ['f3d_ctx.cpp'], hits


def test_library_declares_the_poison_hook():
    lib = f3d.library()
    assert 'f3d_debug_poison' in lib._f3d_symbols and hasattr(lib, 'f3d_debug_poison')
    assert len(lib.f3d_debug_poison.argtypes) == 3 and callable(f3d.Context.debug_poison)
    assert 'int f3d_debug_poison(f3d_ctx* ctx, int byte, int64_t out[2]);' in (ROOT / 'include' / 'f3d.h').read_text()


def test_design_lists_every_policy_key():
    text = (ROOT / 'DESIGN.md').read_text()
    section = text[text.index('### 2.2 Memory a call did not write'):]
    section = section[:section.index('\n## ', 10)] if '\n## ' in section[10:] else section
    for key in POLICY:
        assert f'`{key}`' in section, key
