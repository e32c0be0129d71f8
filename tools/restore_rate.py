#!/usr/bin/env python3
"""Rate of the restore session (lthip_restore_*): a `mixed` tree of 1 MiB files is written by the stream ingest session (one slice, the
images stay in HBM) and restored from those images into a device buffer -- raw (tag 0), LZ4 and zstd stores, each with verify off and
on.  Timed: every lthip_restore_blocks call and lthip_restore_finish (the session's one synchronisation); lthip_restore_create -- the
plan -- is timed by itself.  Beside each figure: the time of the BARE lthip_*_decompress_blocks call over the same blocks into the same
kind of scratch, in the same process -- what the library could already do; the session's overhead (image check, verify, scatter) is the
difference.  The output is compared with the tree once per store.  Recorded into profiles/restore_rate.json: GB/s of output of every
repeat.  There is no threshold.

    python tools/restore_rate.py [--gib 4] [--repeats 3] [--out profiles/restore_rate.json]

--update measures the session with a base instead (lthip_restore_create_from_base / lthip_restore_carry): the same tree is version A and
lies in HBM, version B replaces a share of its files (--share, default one tenth), B's raw (tag 0) blocks are written against a store that
holds A.  Timed: carry + every blocks call + finish, verify off and on, beside a full restore of B (no base, B's full StoreIndex) in the
same process; and the carry alone (verify off), beside a device-to-device torch copy of the same number of bytes in the same process --
that copy, not the code under test, is what the carry is measured against.  Recorded into profiles/restore_update_rate.json.  There is no
threshold.

    python tools/restore_rate.py --update [--share 0.1] [--gib 4] [--repeats 3] [--out profiles/restore_update_rate.json]

--update --in-place measures the update IN PLACE on the same tree (lthip_restore_layout_in_place / lthip_restore_carry_in_place): version A
lies in the buffer that becomes version B.  Three things are timed in one process, alternated repeat by repeat, verify off and on: the
out-of-place update (carry + blocks + finish), the in-place update (carry_in_place + blocks + finish; the buffer is a fresh copy of A every
time, made outside the timing) and the full restore of B.  The out-of-place update of the same process is what the in-place figure is read
against.  Recorded into profiles/restore_update_in_place_rate.json: the three times, in_place_stats, the blocks fetched and the scratch
used.  There is no threshold.

    python tools/restore_rate.py --update --in-place [--share 0.1] [--gib 4] [--repeats 3]

--windows FRACTION measures a window session (lthip_restore_create_windows): the first FRACTION of every file of the same tree, the windows
dense in an output of their own, fed only the blocks the session needs -- beside the full restore of the tree in the same process, the two
alternated repeat by repeat, raw, LZ4 and zstd stores, verify off and on.  Reported per store: the blocks needed, GB/s of output (the
windows' bytes), the milliseconds of the calls behind create, and the plan time (create_windows).  The expectation is a cost that follows
the blocks needed -- a block is decoded whole; the report says what was measured.  Recorded into profiles/restore_windows_rate.json.  There
is no threshold.

    python tools/restore_rate.py --windows 0.25 [--gib 4] [--repeats 3] [--out profiles/restore_windows_rate.json]

--windows FRACTION --cache measures the cache of decoded blocks (BlockCache, lthip_restore_set_cache / lthip_restore_from_cache): 1 /
FRACTION window sessions in one process, each wanting another FRACTION of every file of the same tree.  With a cache the first session
inserts what it is fed and the others are served from the cache; the same sessions run without a cache, alternated repeat by repeat, raw,
LZ4 and zstd stores, verify off and on.  Recorded per session: the milliseconds behind create and set_cache (the inserting session apart
from the served ones), set_cache's own time, and the cache's stats.  Recorded into profiles/restore_cache_rate.json.  There is no threshold.

    python tools/restore_rate.py --windows 0.25 --cache [--gib 4] [--repeats 3] [--out profiles/restore_cache_rate.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FILE = 1 << 20
TAGS = {"none": 0, "lz4": 0x6C7A3432, "zstd": 0x7A746432}


def store_blocks(si):
    h = np.frombuffer(si[:16], np.uint32)
    nb, m = int(h[2]), int(h[3])
    o = 16
    hashes = np.frombuffer(si[o : o + nb * 8], np.uint64).copy()
    o += nb * 8 + m * 8
    first = np.frombuffer(si[o : o + nb * 4], np.uint32).astype(np.int64)
    count = np.frombuffer(si[o + nb * 4 : o + nb * 8], np.uint32).astype(np.int64)
    o += nb * 12
    sizes = np.frombuffer(si[o : o + m * 4], np.uint32).astype(np.int64)
    cs = np.concatenate([[0], np.cumsum(sizes)])
    return hashes, count, cs[first + count] - cs[first]


def update_leg(args):
    import torch

    from bench import KINDS, asset_seeds, make_tree
    from longtail_amd.lib import Context, Ingest, IngestStream, Restore, Store, chunker_params, load

    lib = load()
    dev = torch.device("cuda", 0)
    ctx = Context(0, lib=lib)
    nfiles = int(args.gib * (1 << 30)) // FILE
    n = nfiles * FILE
    mn, av, mx = chunker_params(args.target_chunk_size)
    p_off, p_size = np.arange(nfiles, dtype=np.uint64) * np.uint64(FILE), np.full(nfiles, FILE, np.uint64)
    u8 = dict(dtype=torch.uint8, device=dev)
    seeds = asset_seeds(0x10C0FFEE, 0, nfiles)
    data_a = torch.empty(n + 256, **u8)
    ctx.synth_fill(data_a, p_off, p_size, seeds, KINDS["mixed"])
    replaced = np.arange(0, nfiles, max(1, round(1 / args.share)))
    data_b = data_a.clone()
    ctx.synth_fill(data_b, p_off[replaced], p_size[replaced], asset_seeds(0xB0B0CAFE, 0, len(replaced)), KINDS["mixed"])
    ctx.sync()
    tree = make_tree("files", n, FILE)
    whole, _keep = Ingest.tree(tree["sizes"], tree["path_offsets"], tree["perms"], tree["path_data"], np.arange(nfiles, dtype=np.uint32),
                               np.zeros(nfiles + 1, np.uint64))
    plan = ctx.make_plan(p_off, p_size, mn, av, mx)

    def ingest(data, store):
        """-> (vi, si, [(images, hashes, offsets, sizes)]) of the tree in `data`, raw blocks, one slice"""
        total, d_off, d_len, d_hash, d_first = ctx.chunk_hash(plan, data)
        vi_cap = int(lib.dll.lthip_version_index_size(nfiles, total, total, len(tree["path_data"]))) + 64
        h_vi, h_si = torch.empty(vi_cap, dtype=torch.uint8).pin_memory(), torch.empty(16 + 32 * total + 64, dtype=torch.uint8).pin_memory()
        st = IngestStream(ctx, whole, args.target_chunk_size, args.block_size, args.max_chunks_per_block, "none")
        if store is not None:
            st.set_store(store)
        arena, tail = torch.empty(st.arena_bound(n, total), **u8), torch.empty(st.arena_bound(0, 0), **u8)
        st.slice(0, nfiles, data, d_off, d_len, d_hash, d_first, total, arena)
        _, offs0, sizes0 = st.images()
        offs0, sizes0 = offs0.copy(), sizes0.copy()
        res = st.finish(tail, h_vi, h_si)
        _, offs1, sizes1 = st.images()
        vi, si = bytes(h_vi.numpy()[: res.version_index_size]), bytes(h_si.numpy()[: res.store_index_size])
        st.close()
        hashes = store_blocks(si)[0]
        stored = int(sizes0.astype(np.int64).sum() + sizes1.astype(np.int64).sum())
        keep = max(64, int((offs0.astype(np.int64) + sizes0.astype(np.int64)).max()) if len(offs0) else 0)
        arena = arena[:keep].clone()  # (the bound is the whole tree's: keep what was written)
        return vi, si, [(arena, hashes[: len(offs0)], offs0, sizes0), (tail, hashes[len(offs0) :], offs1.copy(), sizes1.copy())], stored

    vi_a, si_a, _calls_a, _ = ingest(data_a, None)
    del _calls_a
    store = Store(ctx, 0)
    store.add_index(si_a)
    vi_b, si_missing, calls_missing, stored_missing = ingest(data_b, store)
    _, si_full, calls_full, stored_full = ingest(data_b, None)
    store.close()
    offsets_a, bytes_a = Restore.layout(vi_a, 1, lib)
    offsets_b, bytes_b = Restore.layout(vi_b, 1, lib)
    assert bytes_a == bytes_b == n
    out = torch.empty(n, **u8)
    base = (vi_a, offsets_a, n)  # version A as a restore at align 1 leaves it: the tree's bytes
    report = {"workload": f"{args.gib:g} GiB `mixed` tree ({nfiles} files of 1 MiB) resident in HBM as version A; version B replaces {len(replaced)} "
                          "of the files; raw (tag 0) blocks; B's missing blocks were written against a store that holds A",
              "unit": "GB/s of output (the whole of version B)", "repeats": args.repeats, "files_replaced": int(len(replaced)),
              "stored_bytes_of_the_missing_blocks": stored_missing, "stored_bytes_of_all_blocks": stored_full}

    if args.in_place:
        from longtail_amd.lib import restore_layout_in_place

        offsets_ip, bytes_ip, kept_assets = restore_layout_in_place(vi_a, offsets_a, n, vi_b, 1, lib)
        assert bytes_ip == n
        report["unit"] = "milliseconds of carry + every blocks call + finish; GB/s of output (the whole of version B)"
        report["assets_kept_by_the_layout"] = kept_assets

        def once(kind, verify):
            """-> (ms of the calls behind create, finish's result, the session's in_place_stats and scratch bound)"""
            in_place, with_base = kind == "in_place", kind != "full_restore"
            offs = offsets_ip if in_place else offsets_b
            vi, si, calls = (vi_b, si_missing, calls_missing) if with_base else (vi_b, si_full, calls_full)
            dst = data_a[:n].clone() if in_place else out
            if not in_place:
                out.fill_(0xA5)
            rs = Restore(ctx, vi, si, offs, n, verify=verify, base=base if with_base else None)
            stats, bound = rs.in_place_stats(), rs.in_place_scratch_bound()
            scratch = torch.empty(bound, **u8) if in_place and bound else None
            ctx.sync()
            t0 = time.perf_counter()
            if in_place:
                rs.carry_in_place(dst, scratch)
            elif with_base:
                rs.carry(data_a, dst)
            for images, h, o, z in calls:
                if len(h):
                    rs.blocks(h, images, o, z, None, dst)
            code, result = rs.finish()
            ms = (time.perf_counter() - t0) * 1e3
            assert code == 0 and result.bytes_written == n, (code, result.bytes_written)
            if in_place:  # asset a of B at offsets_ip[a]: every file has 1 MiB, so the windows are the tree's in some order
                for a in np.random.default_rng(1).choice(nfiles, 64, replace=False).tolist() + replaced[:8].tolist():
                    assert torch.equal(dst[int(offs[a]) : int(offs[a]) + FILE], data_b[a * FILE : (a + 1) * FILE]), a
                if np.array_equal(offs, offsets_b):
                    assert torch.equal(dst, data_b[:n]), "the buffer differs from version B"
            else:
                assert torch.equal(dst, data_b[:n]), "the restored bytes differ from version B"
            rs.close()
            return ms, result, stats, bound

        kinds = ("update_out_of_place", "in_place", "full_restore")
        for verify in (False, True):
            ms = {k: [] for k in kinds}
            info = {}
            for rep in range(args.repeats + 1):  # (the first is the warm-up: workspaces of the context)
                for k in kinds:
                    t, result, stats, bound = once(k, verify)
                    info[k] = (result, stats, bound)
                    if rep:
                        ms[k].append(round(t, 3))
            entry = {}
            for k in kinds:
                med = float(np.median(ms[k]))
                entry[k] = {"ms": ms[k], "ms_median": med, "GBps_median": round(n / (med * 1e-3) / 1e9, 2), "blocks_fetched": int(info[k][0].blocks_needed)}
            stats, bound = info["in_place"][1], info["in_place"][2]
            entry["in_place"].update(in_place_stats=dict(zip(("kept_occurrences", "kept_bytes", "moved_occurrences", "moved_bytes"), stats)),
                                     scratch_bytes=bound, moved_share_of_the_base_fed_bytes=round(stats[3] / max(1, stats[1] + stats[3]), 4))
            entry["in_place_over_out_of_place"] = round(entry["in_place"]["ms_median"] / entry["update_out_of_place"]["ms_median"], 3)
            report["verify" if verify else "no_verify"] = entry
            print("verify" if verify else "no_verify", json.dumps(entry), flush=True)
        plan.close()
        ctx.close()
        path = Path(args.out if args.out else ROOT / "profiles" / "restore_update_in_place_rate.json")
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(report, indent=1) + "\n")
        print("wrote", path)
        return

    def timed(label, vi, si, calls, with_base, verify):
        plans, rates, result = [], [], None
        for rep in range(args.repeats + 1):  # (the first is the warm-up: workspaces of the context)
            out.fill_(0xA5)
            ctx.sync()
            t0 = time.perf_counter()
            rs = Restore(ctx, vi, si, offsets_b, n, verify=verify, base=base if with_base else None)
            t1 = time.perf_counter()
            if with_base:
                rs.carry(data_a, out)
            for images, h, o, z in calls:
                if len(h):
                    rs.blocks(h, images, o, z, None, out)
            code, result = rs.finish()
            t2 = time.perf_counter()
            assert code == 0 and result.bytes_written == n, (code, result.bytes_written)
            if rep == 0:
                assert torch.equal(out, data_b[:n]), "the restored bytes differ from version B"
            else:
                plans.append(round((t1 - t0) * 1e3, 2))
                rates.append(round(n / (t2 - t1) / 1e9, 2))
            rs.close()
        report[label] = {"GBps": rates, "GBps_median": float(np.median(rates)), "create_ms": plans, "blocks_needed": int(result.blocks_needed),
                         "base_occurrences": int(result.base_occurrences), "occurrences": int(result.occurrences),
                         "base_bytes": int(result.base_bytes)}
        print(label, json.dumps(report[label]), flush=True)
        return result

    for verify in (False, True):
        v = "verify" if verify else "no_verify"
        res = timed(f"update_{v}", vi_b, si_missing, calls_missing, True, verify)
        timed(f"full_restore_{v}", vi_b, si_full, calls_full, False, verify)
    # ---- the carry alone, beside a device-to-device copy of as many bytes ----
    carried = int(res.base_bytes)
    carry_ms, copy_ms = [], []
    for rep in range(args.repeats + 1):
        rs = Restore(ctx, vi_b, si_missing, offsets_b, n, verify=False, base=base)
        ctx.sync()
        t0 = time.perf_counter()
        rs.carry(data_a, out)
        ctx.sync()
        t1 = time.perf_counter()
        rs.close()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        out[:carried].copy_(data_a[:carried])
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if rep:
            carry_ms.append(round((t1 - t0) * 1e3, 3))
            copy_ms.append(round((t3 - t2) * 1e3, 3))
    gbps = lambda ms: round(carried / (float(np.median(ms)) * 1e-3) / 1e9, 2)
    report["carry_alone"] = {"bytes": carried, "ms": carry_ms, "GBps_median": gbps(carry_ms), "torch_copy_ms": copy_ms,
                             "torch_copy_GBps_median": gbps(copy_ms), "carry_over_copy": round(gbps(carry_ms) / gbps(copy_ms), 3)}
    print("carry_alone", json.dumps(report["carry_alone"]), flush=True)
    plan.close()
    ctx.close()
    path = Path(args.out if args.out else ROOT / "profiles" / "restore_update_rate.json")
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(report, indent=1) + "\n")
    print("wrote", path)


def windows_leg(args):
    import torch

    from bench import KINDS, asset_seeds, make_tree
    from longtail_amd.lib import Context, Ingest, IngestStream, Restore, chunker_params, load

    lib = load()
    dev = torch.device("cuda", 0)
    ctx = Context(0, lib=lib)
    nfiles = int(args.gib * (1 << 30)) // FILE
    n = nfiles * FILE
    wlen = max(1, min(FILE, int(FILE * args.windows)))
    wn = nfiles * wlen
    mn, av, mx = chunker_params(args.target_chunk_size)
    p_off, p_size = np.arange(nfiles, dtype=np.uint64) * np.uint64(FILE), np.full(nfiles, FILE, np.uint64)
    u8 = dict(dtype=torch.uint8, device=dev)
    data = torch.empty(n + 256, **u8)
    ctx.synth_fill(data, p_off, p_size, asset_seeds(0x10C0FFEE, 0, nfiles), KINDS["mixed"])
    plan = ctx.make_plan(p_off, p_size, mn, av, mx)
    total, d_off, d_len, d_hash, d_first = ctx.chunk_hash(plan, data)
    tree = make_tree("files", n, FILE)
    whole, _keep = Ingest.tree(tree["sizes"], tree["path_offsets"], tree["perms"], tree["path_data"], np.arange(nfiles, dtype=np.uint32),
                               np.zeros(nfiles + 1, np.uint64))
    vi_cap = int(lib.dll.lthip_version_index_size(nfiles, total, total, len(tree["path_data"]))) + 64
    h_vi, h_si = torch.empty(vi_cap, dtype=torch.uint8).pin_memory(), torch.empty(16 + 32 * total + 64, dtype=torch.uint8).pin_memory()
    out = torch.empty(n, **u8)
    want = data[:n].view(nfiles, FILE)[:, :wlen].reshape(-1)  # the windows, dense
    windows = np.stack([np.arange(nfiles), np.zeros(nfiles), np.full(nfiles, wlen), np.arange(nfiles) * wlen], axis=1).astype(np.uint64)
    report = {"workload": f"{args.gib:g} GiB `mixed` tree ({nfiles} files of 1 MiB), written by lthip_ingest_stream in one slice; the window session "
                          f"restores the first {wlen} bytes of every file ({wlen / FILE:.4g} of the tree) from the blocks it needs, the full session "
                          "the whole tree, alternated in one process: all lthip_restore_blocks calls + lthip_restore_finish",
              "unit": "GB/s of output (windows: the windows' bytes; full: the tree's bytes)", "repeats": args.repeats, "fraction": wlen / FILE,
              "stores": {}}
    for codec, tag in TAGS.items():
        st = IngestStream(ctx, whole, args.target_chunk_size, args.block_size, args.max_chunks_per_block, codec, compression_type=tag or None)
        arena, tail = torch.empty(st.arena_bound(n, total), **u8), torch.empty(st.arena_bound(0, 0), **u8)
        st.slice(0, nfiles, data, d_off, d_len, d_hash, d_first, total, arena)
        _, offs0, sizes0 = st.images()
        offs0, sizes0 = offs0.copy(), sizes0.copy()
        res = st.finish(tail, h_vi, h_si)
        _, offs1, sizes1 = st.images()
        offs1, sizes1 = offs1.copy(), sizes1.copy()
        vi, si = bytes(h_vi.numpy()[: res.version_index_size]), bytes(h_si.numpy()[: res.store_index_size])
        st.close()
        hashes, counts, raws = store_blocks(si)
        calls = [(arena, hashes[: len(offs0)], offs0, sizes0), (tail, hashes[len(offs0) :], offs1, sizes1)]
        offsets, out_bytes = Restore.layout(vi, 1, lib)
        assert out_bytes == n
        entry = {"blocks": int(res.blocks), "raw_bytes_of_the_blocks": int(raws.sum())}
        scratch = torch.empty(max(64, int(((raws + 63) // 64 * 64).sum()) if tag else 64), **u8)  # (room for every block of a call)

        def once(kind, verify):
            """-> (ms of create, ms of the blocks calls + finish, the result)"""
            out.fill_(0xA5)
            ctx.sync()
            t0 = time.perf_counter()
            if kind == "windows":
                rs = Restore(ctx, vi, si, None, wn, verify=verify, windows=windows)
            else:
                rs = Restore(ctx, vi, si, offsets, n, verify=verify)
            t1 = time.perf_counter()
            needed = set(rs.needed_blocks().tolist()) if kind == "windows" else None
            ctx.sync()
            t2 = time.perf_counter()
            for images, h, o, z in calls:
                pick = np.array([x in needed for x in h.tolist()], bool) if needed is not None else np.ones(len(h), bool)
                if pick.any():
                    rs.blocks(h[pick], images, o[pick], z[pick], scratch, out)
            code, result = rs.finish()
            t3 = time.perf_counter()
            nbytes = wn if kind == "windows" else n
            assert code == 0 and result.bytes_written == nbytes, (code, result.bytes_written)
            assert torch.equal(out[:nbytes], want if kind == "windows" else data[:n]), "the restored bytes differ from the tree"
            rs.close()
            return (t1 - t0) * 1e3, (t3 - t2) * 1e3, result

        for verify in (False, True):
            ms = {k: [] for k in ("windows", "full")}
            plans = {k: [] for k in ms}
            results = {}
            for rep in range(args.repeats + 1):  # (the first is the warm-up: workspaces of the context)
                for k in ms:
                    create_ms, run_ms, results[k] = once(k, verify)
                    if rep:
                        plans[k].append(round(create_ms, 2))
                        ms[k].append(round(run_ms, 3))
            v = {}
            for k, nbytes in (("windows", wn), ("full", n)):
                med = float(np.median(ms[k]))
                v[k] = {"ms": ms[k], "ms_median": med, "GBps_median": round(nbytes / (med * 1e-3) / 1e9, 2), "create_ms": plans[k],
                        "blocks_needed": int(results[k].blocks_needed), "occurrences": int(results[k].occurrences),
                        "decoded_bytes": int(results[k].decoded_bytes)}
            v["windows_over_full_ms"] = round(v["windows"]["ms_median"] / v["full"]["ms_median"], 3)
            v["blocks_needed_over_all"] = round(v["windows"]["blocks_needed"] / max(1, v["full"]["blocks_needed"]), 3)
            entry["verify" if verify else "no_verify"] = v
        report["stores"][codec] = entry
        print(codec, json.dumps(entry), flush=True)
        del arena, tail, scratch
    plan.close()
    ctx.close()
    path = Path(args.out if args.out else ROOT / "profiles" / "restore_windows_rate.json")
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(report, indent=1) + "\n")
    print("wrote", path)


def cache_leg(args):
    """--windows FRACTION --cache: 1 / FRACTION window sessions in one process, each wanting another FRACTION of every file, with a
    BlockCache (the first session inserts, the others are served) and without one, alternated repeat by repeat."""
    import torch

    from bench import KINDS, asset_seeds, make_tree
    from longtail_amd.lib import BlockCache, Context, Ingest, IngestStream, Restore, chunker_params, load

    lib = load()
    dev = torch.device("cuda", 0)
    ctx = Context(0, lib=lib)
    nfiles = int(args.gib * (1 << 30)) // FILE
    n = nfiles * FILE
    wlen = max(1, min(FILE, int(FILE * args.windows)))
    passes = max(1, FILE // wlen)
    wn = nfiles * wlen
    mn, av, mx = chunker_params(args.target_chunk_size)
    p_off, p_size = np.arange(nfiles, dtype=np.uint64) * np.uint64(FILE), np.full(nfiles, FILE, np.uint64)
    u8 = dict(dtype=torch.uint8, device=dev)
    data = torch.empty(n + 256, **u8)
    ctx.synth_fill(data, p_off, p_size, asset_seeds(0x10C0FFEE, 0, nfiles), KINDS["mixed"])
    plan = ctx.make_plan(p_off, p_size, mn, av, mx)
    total, d_off, d_len, d_hash, d_first = ctx.chunk_hash(plan, data)
    tree = make_tree("files", n, FILE)
    whole, _keep = Ingest.tree(tree["sizes"], tree["path_offsets"], tree["perms"], tree["path_data"], np.arange(nfiles, dtype=np.uint32),
                               np.zeros(nfiles + 1, np.uint64))
    vi_cap = int(lib.dll.lthip_version_index_size(nfiles, total, total, len(tree["path_data"]))) + 64
    h_vi, h_si = torch.empty(vi_cap, dtype=torch.uint8).pin_memory(), torch.empty(16 + 32 * total + 64, dtype=torch.uint8).pin_memory()
    out = torch.empty(wn, **u8)
    files = data[:n].view(nfiles, FILE)
    want = [files[:, q * wlen : (q + 1) * wlen].reshape(-1) for q in range(passes)]
    windows = [np.stack([np.arange(nfiles), np.full(nfiles, q * wlen), np.full(nfiles, wlen), np.arange(nfiles) * wlen], axis=1).astype(np.uint64)
               for q in range(passes)]
    report = {"workload": f"{args.gib:g} GiB `mixed` tree ({nfiles} files of 1 MiB), written by lthip_ingest_stream in one slice; {passes} window "
                          f"sessions in one process, session q restores bytes [q, q + 1) x {wlen} of every file.  With a cache (one slot per "
                          "block, slots of the largest block's raw size) the first session inserts what it is fed and the others are served "
                          "from the cache; without one every session is fed the blocks it needs.  Alternated repeat by repeat.",
              "unit": "milliseconds of a session behind create and set_cache: every blocks call + from_cache + finish", "repeats": args.repeats,
              "fraction": wlen / FILE, "sessions": passes, "stores": {}}
    for codec, tag in TAGS.items():
        st = IngestStream(ctx, whole, args.target_chunk_size, args.block_size, args.max_chunks_per_block, codec, compression_type=tag or None)
        arena, tail = torch.empty(st.arena_bound(n, total), **u8), torch.empty(st.arena_bound(0, 0), **u8)
        st.slice(0, nfiles, data, d_off, d_len, d_hash, d_first, total, arena)
        _, offs0, sizes0 = st.images()
        offs0, sizes0 = offs0.copy(), sizes0.copy()
        res = st.finish(tail, h_vi, h_si)
        _, offs1, sizes1 = st.images()
        offs1, sizes1 = offs1.copy(), sizes1.copy()
        vi, si = bytes(h_vi.numpy()[: res.version_index_size]), bytes(h_si.numpy()[: res.store_index_size])
        st.close()
        hashes, counts, raws = store_blocks(si)
        calls = [(arena, hashes[: len(offs0)], offs0, sizes0), (tail, hashes[len(offs0) :], offs1, sizes1)]
        entry = {"blocks": int(res.blocks), "raw_bytes_of_the_blocks": int(raws.sum()), "slots": int(len(raws)), "slot_bytes": int(raws.max())}
        scratch = torch.empty(max(64, int(((raws + 63) // 64 * 64).sum()) if tag else 64), **u8)  # (room for every block of a call)

        def once(q, verify, cache):
            """-> (ms of set_cache, ms of the calls behind it, the result, the session's cache stats)"""
            out.fill_(0xA5)
            rs = Restore(ctx, vi, si, None, wn, verify=verify, windows=windows[q])
            ctx.sync()
            t0 = time.perf_counter()
            if cache is not None:
                rs.set_cache(cache)
            needed = set(rs.needed_blocks().tolist())
            ctx.sync()
            t1 = time.perf_counter()
            for images, h, o, z in calls:
                pick = np.array([x in needed for x in h.tolist()], bool)
                if pick.any():
                    rs.blocks(h[pick], images, o[pick], z[pick], scratch, out)
            if cache is not None:
                rs.from_cache(out)
            code, result = rs.finish()
            t2 = time.perf_counter()
            assert code == 0 and result.bytes_written == wn, (code, result.bytes_written)
            assert torch.equal(out, want[q]), "the restored bytes differ from the tree"
            stats = rs.cache_stats()
            rs.close()
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3, result, stats

        for verify in (False, True):
            ms = {k: [[] for _ in range(passes)] for k in ("cache", "no_cache")}
            attach, stats, cache_stats = [], None, None
            for rep in range(args.repeats + 1):  # (the first is the warm-up: workspaces of the context)
                cache = BlockCache(ctx, len(raws), int(raws.max()))
                for k in ("cache", "no_cache"):
                    for q in range(passes):
                        a_ms, run_ms, result, s = once(q, verify, cache if k == "cache" else None)
                        if rep:
                            ms[k][q].append(round(run_ms, 3))
                            if k == "cache" and q:
                                attach.append(round(a_ms, 3))
                        if k == "cache" and q == passes - 1:
                            stats = s
                cache_stats = cache.stats()
                cache.close()
            med = lambda rows: float(np.median([x for r in rows for x in r]))
            v = {"inserting_session_ms": ms["cache"][0], "served_sessions_ms": ms["cache"][1:], "no_cache_first_session_ms": ms["no_cache"][0],
                 "no_cache_other_sessions_ms": ms["no_cache"][1:], "set_cache_ms_of_the_served_sessions": attach,
                 "inserting_session_ms_median": med(ms["cache"][:1]), "served_session_ms_median": med(ms["cache"][1:]) if passes > 1 else None,
                 "no_cache_first_session_ms_median": med(ms["no_cache"][:1]),
                 "no_cache_other_session_ms_median": med(ms["no_cache"][1:]) if passes > 1 else None,
                 "last_served_session_cache_stats": dict(zip(("fed_blocks", "fed_bytes", "inserted", "bypassed", "dropped", "fed_entries"), stats)),
                 "cache_stats": cache_stats}
            v["inserting_over_no_cache"] = round(v["inserting_session_ms_median"] / v["no_cache_first_session_ms_median"], 3)
            entry["verify" if verify else "no_verify"] = v
        report["stores"][codec] = entry
        print(codec, json.dumps(entry), flush=True)
        del arena, tail, scratch
    plan.close()
    ctx.close()
    path = Path(args.out if args.out else ROOT / "profiles" / "restore_cache_rate.json")
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(report, indent=1) + "\n")
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--target-chunk-size", type=int, default=65536)
    ap.add_argument("--block-size", type=int, default=8 << 20)
    ap.add_argument("--max-chunks-per-block", type=int, default=1024)
    ap.add_argument("--out", default=None, help="default: profiles/restore_rate.json, with --update profiles/restore_update_rate.json")
    ap.add_argument("--update", action="store_true", help="the session with a base: version A resident, version B restored from it")
    ap.add_argument("--in-place", action="store_true", help="--update: the out-of-place update, the update in place and the full restore, alternated")
    ap.add_argument("--share", type=float, default=0.1, help="--update: the share of the files that version B replaces")
    ap.add_argument("--windows", type=float, default=None, metavar="FRACTION",
                    help="a window session over the first FRACTION of every file, beside the full restore (profiles/restore_windows_rate.json)")
    ap.add_argument("--cache", action="store_true",
                    help="--windows: 1 / FRACTION window sessions with a BlockCache and without one (profiles/restore_cache_rate.json)")
    args = ap.parse_args()
    if args.cache:
        if args.windows is None:
            ap.error("--cache goes with --windows FRACTION")
        return cache_leg(args)
    if args.windows is not None:
        return windows_leg(args)
    if args.update:
        return update_leg(args)
    args.out = args.out or str(ROOT / "profiles" / "restore_rate.json")

    import torch

    from bench import KINDS, asset_seeds, make_tree
    from longtail_amd.lib import Context, Ingest, IngestStream, Restore, chunker_params, load

    lib = load()
    dev = torch.device("cuda", 0)
    ctx = Context(0, lib=lib)
    nfiles = int(args.gib * (1 << 30)) // FILE
    n = nfiles * FILE
    mn, av, mx = chunker_params(args.target_chunk_size)
    p_off, p_size = np.arange(nfiles, dtype=np.uint64) * np.uint64(FILE), np.full(nfiles, FILE, np.uint64)
    u8 = dict(dtype=torch.uint8, device=dev)
    data = torch.empty(n + 256, **u8)
    ctx.synth_fill(data, p_off, p_size, asset_seeds(0x10C0FFEE, 0, nfiles), KINDS["mixed"])
    plan = ctx.make_plan(p_off, p_size, mn, av, mx)
    total, d_off, d_len, d_hash, d_first = ctx.chunk_hash(plan, data)
    tree = make_tree("files", n, FILE)
    whole, _keep = Ingest.tree(tree["sizes"], tree["path_offsets"], tree["perms"], tree["path_data"], np.arange(nfiles, dtype=np.uint32),
                               np.zeros(nfiles + 1, np.uint64))
    vi_cap = int(lib.dll.lthip_version_index_size(nfiles, total, total, len(tree["path_data"]))) + 64
    h_vi, h_si = torch.empty(vi_cap, dtype=torch.uint8).pin_memory(), torch.empty(16 + 32 * total + 64, dtype=torch.uint8).pin_memory()
    out = torch.empty(n, **u8)
    report = {"workload": f"{args.gib:g} GiB `mixed` tree ({nfiles} files of 1 MiB), written by lthip_ingest_stream in one slice, restored from its "
                          "images in HBM into a device buffer: all lthip_restore_blocks calls + lthip_restore_finish",
              "unit": "GB/s of output", "repeats": args.repeats, "stores": {}}
    for codec, tag in TAGS.items():
        st = IngestStream(ctx, whole, args.target_chunk_size, args.block_size, args.max_chunks_per_block, codec, compression_type=tag or None)
        arena, tail = torch.empty(st.arena_bound(n, total), **u8), torch.empty(st.arena_bound(0, 0), **u8)
        st.slice(0, nfiles, data, d_off, d_len, d_hash, d_first, total, arena)
        _, offs0, sizes0 = st.images()
        offs0, sizes0 = offs0.copy(), sizes0.copy()
        res = st.finish(tail, h_vi, h_si)
        _, offs1, sizes1 = st.images()
        offs1, sizes1 = offs1.copy(), sizes1.copy()
        vi, si = bytes(h_vi.numpy()[: res.version_index_size]), bytes(h_si.numpy()[: res.store_index_size])
        st.close()
        hashes, counts, raws = store_blocks(si)
        calls = [(arena, hashes[: len(offs0)], offs0, sizes0), (tail, hashes[len(offs0) :], offs1, sizes1)]
        assert len(hashes) == len(offs0) + len(offs1) == res.blocks
        offsets, out_bytes = Restore.layout(vi, 1, lib)
        assert out_bytes == n
        entry = {"blocks": int(res.blocks), "raw_bytes_of_the_blocks": int(raws.sum()), "stored_bytes": int(sizes0.astype(np.int64).sum() + sizes1.astype(np.int64).sum())}
        scratch = None
        for verify in (False, True):
            plans, rates = [], []
            for rep in range(args.repeats + 1):  # (the first is the warm-up: workspaces of the context)
                out.fill_(0xA5)
                ctx.sync()
                t0 = time.perf_counter()
                rs = Restore(ctx, vi, si, offsets, n, verify=verify)
                t1 = time.perf_counter()
                if scratch is None:
                    bound = max(rs.scratch_bound(h) for _, h, _, _ in calls)
                    scratch = torch.empty(max(bound, 64), **u8)
                    ctx.sync()
                    t1 = time.perf_counter()
                for images, h, o, z in calls:
                    if len(h):
                        rs.blocks(h, images, o, z, scratch, out)
                code, result = rs.finish()
                t2 = time.perf_counter()
                assert code == 0 and result.bytes_written == n, (code, result.bytes_written)
                if rep == 0:
                    assert torch.equal(out, data[:n]), "the restored bytes differ from the tree"
                else:
                    plans.append(round((t1 - t0) * 1e3, 2))
                    rates.append(round(n / (t2 - t1) / 1e9, 2))
                rs.close()
            entry["verify" if verify else "no_verify"] = {"GBps": rates, "GBps_median": float(np.median(rates)), "create_ms": plans}
        if codec != "none":  # the bare decoder call over the same blocks, into the same scratch
            decode = ctx.lz4_decompress_blocks if codec == "lz4" else ctx.zstd_decompress_blocks
            hdr, k, ms = 28 + 12 * counts, 0, []
            for rep in range(args.repeats + 1):
                ctx.sync()
                t0 = time.perf_counter()
                k = 0
                for images, h, o, z in calls:
                    if len(h):
                        r = raws[k : k + len(h)]
                        slots = np.concatenate([[0], np.cumsum((r + 63) // 64 * 64)[:-1]])
                        decode(images, o.astype(np.int64) + hdr[k : k + len(h)], z.astype(np.int64) - hdr[k : k + len(h)], scratch, slots, r)
                        k += len(h)
                ctx.sync()
                if rep:
                    ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            entry["bare_decoder_ms"] = ms  # (it decodes the store's unique bytes once; the session also writes every duplicate)
            entry["bare_decoder_GBps_of_decoded_bytes_median"] = round(int(raws.sum()) / (float(np.median(ms)) * 1e-3) / 1e9, 2)
        report["stores"][codec] = entry
        print(codec, json.dumps(entry), flush=True)
        del arena, tail, scratch
    plan.close()
    ctx.close()
    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(report, indent=1) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
