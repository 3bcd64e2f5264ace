"""Which kernel the ComplEx / HolE 1-vs-K sweep ran for a shape BEFORE csrc/ge_sweep_route.h existed: a restatement of
the chain of launchers that each tried the one that superseded it and fell back on GE_ENOTSUP (ge_rank.hip ->
ge_rank_pipe.hip -> ge_rank_f16.hip, and ge_1vk.hip into the same chain), kept in that nested shape on purpose: it shares
no structure with the route table it checks (tests/test_sweep_route_host.py).  Each launcher returns the name of the
kernel it launched, or an error code.  Below them, in the same way, the fronts of the top-k and candidate-set launchers
and the top-k workspace size as they stood before route_topk, route_masked_rank and topk_ws_bytes moved to that header."""
GE_EINVAL, GE_ENOTSUP = -22, -95
INT32_MAX = 2 ** 31 - 1
KERNELS = ["None", "F16", "Pipe40", "Pipe32", "Pipe24", "RankF32", "ScoreTileF16", "ScoreTile", "ScoreFullK",
           "ScoreBasic"]                      # SweepRoute::Kernel, in the enum's order


def _tiles(n):
    return (n + 127) // 128


def _rank_planes_bytes(N, d, K):
    if d % 8 != 0 or d < 56 or d > 288 or N <= 0 or K <= 0:
        return 0
    kkb = (d + 15) // 16
    plane_bytes = 4 * _tiles(K) * kkb * 2 * 512 * 2
    if plane_bytes >= 1 << 32:
        return 0
    return (N * 4 + 255) // 256 * 256 + plane_bytes


def _f16_launch_kkb(d, B, K):
    n_rb, n_ct, kkb = _tiles(B), _tiles(K), (d + 15) // 16
    if n_ct > INT32_MAX // 8 or n_rb > INT32_MAX // 8:
        return GE_ENOTSUP
    if 4 * n_ct * kkb * 2 * 512 * 2 >= 1 << 32:
        return GE_ENOTSUP
    return "F16"


def _sweep_f16_launch(N, d, B, K, max_norm):
    f16_dim_ok = d % 8 == 0 and d >= 56 and d <= 288 and max_norm <= 8.0
    if not f16_dim_ok or _rank_planes_bytes(N, d, K) == 0:
        return GE_ENOTSUP
    return _f16_launch_kkb(d, B, K)


def _pipe_launch_cw(cw, d, B, K):
    lds = 4 * (128 * (d + 1) + 2 * 128 * (cw + 1) + 3 * 128) + 8 * 128 + 4 * 128 * 4 + 4 * 2 * 128
    if lds > 160 * 1024:
        return GE_ENOTSUP
    if _tiles(K) > INT32_MAX // 2 or _tiles(B) > INT32_MAX // 2:
        return GE_ENOTSUP
    return "Pipe%d" % cw


def _sweep_pipe_launch(N, d, B, K, max_norm):
    rc = _sweep_f16_launch(N, d, B, K, max_norm)
    if rc != GE_ENOTSUP:
        return rc
    if d % 40 == 0:
        return _pipe_launch_cw(40, d, B, K)
    if d % 32 == 0:
        return _pipe_launch_cw(32, d, B, K)
    if d % 24 == 0:
        return _pipe_launch_cw(24, d, B, K)
    return GE_ENOTSUP


def _complex_rank_1vK_launch(N, d, B, K, max_norm, mod16):
    if d <= 0 or d & 7:
        return GE_EINVAL if (d <= 0 or d & 1) else GE_ENOTSUP
    if d > 288:
        return GE_ENOTSUP
    if mod16 != 0:
        return GE_EINVAL
    if B == 0 or K == 0:
        return 0
    rc = _sweep_pipe_launch(N, d, B, K, max_norm)
    if rc != GE_ENOTSUP:
        return rc
    if d > 232:
        return GE_ENOTSUP
    if _tiles(B) > 65535:
        return GE_ENOTSUP
    return "RankF32"


def _complex_score_1vK_launch(N, d, B, K, max_norm, mod16):
    if d <= 0 or d & 1:
        return GE_EINVAL
    if B == 0 or K == 0:
        return 0
    if _tiles(B) * _tiles(K) >= 512 and mod16 == 0:
        rc = _sweep_pipe_launch(N, d, B, K, max_norm)
        if rc != GE_ENOTSUP:
            return rc
    k = d // 2
    big = _tiles(B) * _tiles(K) >= 512
    bm = 128 if big else 64
    gy, gx = (B + bm - 1) // bm, (K + bm - 1) // bm
    if gy > 65535 or gx > 2147483647:
        return GE_ENOTSUP
    if not big and d % 8 == 0 and d >= 56 and d <= 224 and max_norm <= 8.0 and mod16 == 0:
        return "ScoreTileF16"
    if not big and d % 8 == 0 and d <= 256 and mod16 == 0:
        return "ScoreTile"
    KP = (k + 3) & ~3
    fullk_lds = 4 * (2 * 64 * (2 * KP + 1) + 128)
    if not big and fullk_lds <= 150 * 1024:
        return "ScoreFullK"
    return "ScoreBasic"


# ---- the top-k sweep and the candidate-set (masked) forms, BEFORE route_topk / route_masked_rank existed: each launcher
# of ge_rank_f16.hip and ge_rank_f16_masked.hip refused shapes at its own front, restated here launcher by launcher.
# They stop where the launchers first looked at the workspace.
TOPK_MAX_K = 128


def _masked_shape_ok(N, d, B, K, max_norm):
    f16_sweep_ok = d % 8 == 0 and d >= 56 and d <= 288 and max_norm <= 8.0
    return f16_sweep_ok and _rank_planes_bytes(N, d, K) != 0 and _tiles(B) <= INT32_MAX // 8


def _topk_f16_launch(N, d, B, K, max_norm, mod16, k):
    f16_sweep_ok = d % 8 == 0 and d >= 56 and d <= 288 and max_norm <= 8.0
    if not f16_sweep_ok or _rank_planes_bytes(N, d, K) == 0:
        return GE_ENOTSUP
    if k < 1:
        return GE_EINVAL
    if k > TOPK_MAX_K:
        return GE_ENOTSUP
    if B == 0:
        return 0
    return "F16"


def _masked_topk_launch(N, d, B, K, max_norm, mod16, k):
    if not _masked_shape_ok(N, d, B, K, max_norm):
        return GE_ENOTSUP
    if mod16 != 0:
        return GE_EINVAL
    if k < 1:
        return GE_EINVAL
    if k > TOPK_MAX_K:
        return GE_ENOTSUP
    if B == 0:
        return 0
    return "F16"


def _masked_rank_launch(N, d, B, K, max_norm, mod16, k):
    if not _masked_shape_ok(N, d, B, K, max_norm):
        return GE_ENOTSUP
    if mod16 != 0:
        return GE_EINVAL
    if B == 0:          # (never reached the launcher: ge_rank_1vK_masked returned 0 for B == 0 before calling it)
        return 0
    return "F16"


def topk_splits(B, K):
    n_rb, n_ct = _tiles(B), _tiles(K)
    if n_rb >= 256:
        return 1
    return max(1, min(n_ct, (256 + n_rb - 1) // n_rb))


def _topk_ws_rows(n_rb, K, k):
    kp = (k + 95) // 64 * 64
    return n_rb * 128 * topk_splits(n_rb * 128, K) * (kp + 128 + k) * 8


def topk_ws_bytes(B, K, k):
    if B <= 0 or K <= 0 or k < 1 or k > TOPK_MAX_K:
        return 0
    n_rb = _tiles(B)
    need = _topk_ws_rows(n_rb, K, k)
    for r in range(1, min(n_rb, 256)):
        need = max(need, _topk_ws_rows(r, K, k))
    return need + 256


def topk_grid_ok(B, K):
    """the launchers' last refusal, behind the workspace checks: n_rb * ns > INT32_MAX was GE_ENOTSUP"""
    return _tiles(B) * topk_splits(B, K) <= INT32_MAX


_ENTRIES = {"rank": _complex_rank_1vK_launch, "score": _complex_score_1vK_launch, "topk": _topk_f16_launch,
            "masked_topk": _masked_topk_launch, "masked_rank": _masked_rank_launch}


def route(entry, N, d, B, K, max_norm, mod16, k=None):
    """(kernel name, status) of entry "rank", "score", "topk", "masked_rank" or "masked_topk" (the last three take k)."""
    rc = _ENTRIES[entry](N, d, B, K, max_norm, mod16) if k is None else _ENTRIES[entry](N, d, B, K, max_norm, mod16, k)
    return (rc, 0) if isinstance(rc, str) else ("None", rc)
