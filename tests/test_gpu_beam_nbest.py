"""masr_beam_nbest_gpu / masr_gbeam_nbest: the N best prefixes of the GPU prefix search, read from what the search left on the device.

* entry 0 is the search's own result BIT for bit (LM-free and with a character scorer of order 3), count = min(nbest, live set);
* an utterance's n-best does not depend on its neighbours in the batch;
* against the host-thread search on the same candidates (masr_beam_search_batch_nbest, nbest = min(10, beam)).  The two searches
  agree only to TOL(s) = 1e-3 * max(1, |s|) (the bound of tests/test_beam_search.py), so ranks are only comparable where the host's
  own scores are further apart than that: a rank whose host score differs from both host neighbours by more than 2 TOL is compared
  rank by rank (tokens equal, score within TOL); the ranks of a tighter cluster are compared as a set; a cluster that straddles
  rank nbest cannot be compared and is left out -- at most 10 % of all ranks of the HOST_SHAPES and REVIVED cases (asserted; their seeds were
  chosen on the host search alone, which needs no GPU);
* streams: after every 16-frame chunk entry 0 is the advance's own result, at the end the rows are the offline ones (cluster rule);
* the refusals, by name."""
import ctypes as C

import numpy as np
import pytest

from tests.test_beam_search import _lm_decoder

# seed, V, frames per utterance, beam, cutoff_prob, cutoff_top_n, Dirichlet concentration: the cases of
# test_beam_search.py::test_gpu_prefix_search_matches_host_search without its 4233-word one -- what the bit-exact tests run on
SHAPES = [(0, 6, (12, 5, 9), 4, 1.0, 40, 0.4), (1, 50, (30, 30), 8, 0.99, 5, 0.4), (2, 300, (60, 41, 1), 20, 0.99, 40, 0.05),
          (3, 5, (40,), 300, 1.0, 40, 0.4), (5, 600, (90, 64), 64, 0.95, 64, 0.01)]
# The host comparison alone takes other seeds and, for the 300- and 600-word cases, another concentration: at 0.05 / 0.01 their ten
# best score around -100 within 0.2 of each other -- one cluster under 2 TOL that straddles rank 10 for every seed tried (0 .. 59),
# i.e. nothing the two searches could be compared on.  At 0.002 the posteriors are as peaked as a trained model's and the host's own
# scores separate.
HOST_SHAPES = [SHAPES[0], SHAPES[1], (7, 300, (60, 41, 1), 20, 0.99, 40, 0.002), (4, 5, (40,), 300, 1.0, 40, 0.4),
               (7, 600, (90, 64), 64, 0.95, 64, 0.002)]
REVIVED = [(0, 2), (1, 3), (2, 5), (3, 10), (4, 10), (5, 16)]         # test_gpu_prefix_search_small_beam_revived_prefixes


def shape_probs(seed, V, Ts, conc):
    rng = np.random.default_rng(seed)
    return [rng.dirichlet(np.ones(V) * conc, size=T).astype(np.float32) for T in Ts]


def revived_probs(seed):
    rng = np.random.default_rng(100 + seed)
    V, T = 24, 150
    alpha = np.full(V, 0.03)
    alpha[[0, 3, 7]] = 1.5
    return [rng.dirichlet(alpha, size=T).astype(np.float32), rng.dirichlet(alpha, size=T // 2).astype(np.float32)]


def all_cases(shapes=None):
    """(name, probabilities, beam, cutoff_prob, cutoff_top_n) of every case of this file"""
    out = [(f'V{V}', shape_probs(seed, V, Ts, conc), beam, cut, topn)
           for seed, V, Ts, beam, cut, topn, conc in (SHAPES if shapes is None else shapes)]
    return out + [(f'revived{seed}', revived_probs(seed), beam, 0.99, 40) for seed, beam in REVIVED]


def tol(s):
    return 1e-3 * max(1.0, abs(s))


def clusters(host_scores, n):
    """host scores best first (one more than n where the host has it) -> ([(lo, hi)] rank ranges to compare, ranks left out).
    Neighbouring ranks belong to one cluster when their host scores are within 2 TOL; a cluster reaching past rank n - 1 is left
    out."""
    m = len(host_scores)
    keep, left, lo = [], 0, 0
    for r in range(1, m + 1):
        if r < m and abs(host_scores[r] - host_scores[r - 1]) <= 2 * tol(host_scores[r - 1]):
            continue
        if lo < n:
            if r <= n:
                keep.append((lo, r))
            else:
                left += n - lo
        lo = r
    return keep, left


def compare(gpu, host, n):
    """gpu / host: [(token ids, score)] best first (host: up to n + 1 entries) -> (ranks compared or left out, ranks left out)"""
    host = [h for h in host if h[1] > -np.inf]     # (the host trie keeps prefixes of probability zero; the GPU search drops them)
    assert len(gpu) == min(n, len(host))
    keep, left = clusters([s for _, s in host], len(gpu))
    for lo, hi in keep:
        g, h = gpu[lo:hi], host[lo:hi]
        assert sorted(tuple(t) for t, _ in g) == sorted(tuple(t) for t, _ in h), (lo, hi, g, h)
        if hi - lo == 1:
            assert abs(g[0][1] - h[0][1]) <= tol(h[0][1]), (lo, g, h)
        else:
            hs = dict((tuple(t), s) for t, s in h)
            for t, s in g:
                assert abs(s - hs[tuple(t)]) <= tol(hs[tuple(t)]), (lo, hi, t, s, hs[tuple(t)])
    return len(gpu), left


def _decoder(V, beam, cut, topn):
    from masr_amd.decoders.beam_search_decoder import BeamSearchDecoder
    vocab = ['<blank>'] + [chr(0x4e00 + i) for i in range(V - 1)]
    return BeamSearchDecoder(alpha=0, beta=0, beam_size=beam, cutoff_prob=cut, cutoff_top_n=topn, vocab_list=vocab, num_processes=4,
                             language_model_path=None)


def _stack(probs):
    B, Ts, V = len(probs), max(p.shape[0] for p in probs), probs[0].shape[1]
    stacked = np.zeros((B, Ts, V), np.float32)
    for i, p in enumerate(probs):
        stacked[i, :p.shape[0]] = p
    return stacked, np.array([p.shape[0] for p in probs], np.int32), B, Ts, V


def gpu_search_and_nbest(dec, probs, n):
    """the decoder's own launches: pruning, masr_beam_search_gpu_lm, masr_beam_nbest_gpu -> the search's packed rows [B, max_len +
    2], the n-best rows [B, n, max_len + 2], counts [B] (host int32 arrays), max_len"""
    from masr_amd import runtime
    stacked, frames, B, Ts, V = _stack(probs)
    assert dec.gpu_search_supported(Ts, V)
    eng = runtime.aux_engine()
    packed, max_len, keep = dec._search_gpu(eng, dec._candidates(stacked.reshape(B * Ts, V), to_host=False), frames, B, Ts)
    flat, keep_n = dec._nbest_gpu(eng, B, max_len, n)
    flat = flat.cpu().numpy()
    return packed.cpu().numpy(), flat[:B * n * (max_len + 2)].reshape(B, n, max_len + 2), flat[B * n * (max_len + 2):], max_len


def entry0_is_the_search_result(one, rows, count, max_len, n, beam):
    for b in range(one.shape[0]):
        L = one[b, max_len]
        assert 1 <= count[b] <= min(n, beam)
        assert rows[b, 0, max_len] == L and rows[b, 0, max_len + 1] == one[b, max_len + 1]          # length, score bits
        assert np.array_equal(rows[b, 0, :L], one[b, :L])
        sc = rows[b, :, max_len + 1].copy().view(np.float32)
        assert (rows[b, count[b]:, max_len] == 0).all() and np.isneginf(sc[count[b]:]).all()
        assert len({tuple(rows[b, r, :rows[b, r, max_len]]) for r in range(count[b])}) == count[b]  # distinct prefixes


@pytest.mark.gpu
@pytest.mark.parametrize('case', range(len(SHAPES) + len(REVIVED)))
def test_entry_0_is_the_search_result_and_count_is_the_live_set(case):
    name, probs, beam, cut, topn = all_cases()[case]
    dec = _decoder(probs[0].shape[1], beam, cut, topn)
    for n in sorted({1, min(10, beam), beam}):
        one, rows, count, max_len = gpu_search_and_nbest(dec, probs, n)
        entry0_is_the_search_result(one, rows, count, max_len, n, beam)
        if name == 'V5':
            # beam 300 over 5 characters: 40 frames fill the beam, but over the first 3 frames there are at most 1 + 4 + 16 + 64 = 85
            # prefixes -- a live set smaller than the beam, and count is its size
            short = [probs[0][:3]]
            full = gpu_search_and_nbest(dec, short, beam)[2]
            one, rows, count, max_len = gpu_search_and_nbest(dec, short, n)
            entry0_is_the_search_result(one, rows, count, max_len, n, beam)
            assert 1 <= full[0] <= 85 and count[0] == min(n, full[0])


@pytest.mark.gpu
@pytest.mark.parametrize('case', range(len(SHAPES) + len(REVIVED)))
def test_entry_0_with_a_language_model_is_the_search_result(tmp_path, case):
    """the same cases with a character ARPA model of order 3 bound: every row's score is the decoder's approx_ctc"""
    name, probs, beam, cut, topn = all_cases()[case]
    V = probs[0].shape[1]
    dec, vocab, _ = _lm_decoder(tmp_path, V, beam, cut, topn, order=3)
    for n in sorted({1, min(10, beam), beam}):
        one, rows, count, max_len = gpu_search_and_nbest(dec, probs, n)
        entry0_is_the_search_result(one, rows, count, max_len, n, beam)
    # the scorer is live in the reported scores: the LM-free rows of the same posteriors differ
    plain = gpu_search_and_nbest(_decoder(V, beam, cut, topn), probs, 1)[1]
    assert not np.array_equal(plain[:, 0, max_len + 1], rows[:, 0, max_len + 1])


@pytest.mark.gpu
def test_an_utterances_nbest_does_not_depend_on_its_neighbours():
    for name, probs, beam, cut, topn in all_cases()[1:3]:
        dec = _decoder(probs[0].shape[1], beam, cut, topn)
        n = min(10, beam)
        rng = np.random.default_rng(9)
        V = probs[0].shape[1]
        others = [rng.dirichlet(np.ones(V) * 0.3, size=T).astype(np.float32) for T in (probs[0].shape[0] + 7, 3)]
        _, alone, c1, m1 = gpu_search_and_nbest(dec, [probs[0]], n)
        _, third, c3, m3 = gpu_search_and_nbest(dec, others + [probs[0]], n)
        assert c1[0] == c3[2]
        for r in range(c1[0]):
            L = alone[0, r, m1]
            assert third[2, r, m3] == L and third[2, r, m3 + 1] == alone[0, r, m1 + 1]
            assert np.array_equal(third[2, r, :L], alone[0, r, :L])


def host_nbest(dec, probs, n):
    """masr_beam_search_batch_nbest on the candidates the GPU pruning gives (the GPU search's own input)"""
    stacked, frames, B, Ts, V = _stack(probs)
    idx, logp, cnt, _, K = dec._candidates(stacked.reshape(B * Ts, V))
    return dec._search_host_nbest(idx, logp, cnt, frames, B, Ts, K, n, True)


@pytest.mark.gpu
def test_nbest_against_the_host_search_on_the_same_candidates():
    ranks = left = 0
    for name, probs, beam, cut, topn in all_cases(HOST_SHAPES):
        dec = _decoder(probs[0].shape[1], beam, cut, topn)
        n = min(10, beam)
        one, rows, count, max_len = gpu_search_and_nbest(dec, probs, n)
        host = host_nbest(dec, probs, min(n + 1, beam))
        for b in range(len(probs)):
            gpu = [(rows[b, r, :rows[b, r, max_len]].tolist(), float(rows[b, r, max_len + 1:].copy().view(np.float32)[0]))
                   for r in range(count[b])]
            a, l = compare(gpu, host[b], n)
            print(f'{name} utterance {b}: {a} ranks, {l} left out')
            ranks, left = ranks + a, left + l
    print(f'{left} of {ranks} ranks left out')
    assert left <= 0.10 * ranks


@pytest.mark.gpu
@pytest.mark.parametrize('beam', [5, 300])
def test_stream_nbest_is_the_advance_result_and_the_offline_nbest(beam):
    from masr_amd import _lib
    rng = np.random.default_rng(77)
    V, T = 60, 131
    alpha = np.full(V, 0.02)
    alpha[[0, 5, 9, 11]] = 1.0
    probs = rng.dirichlet(alpha, size=T).astype(np.float32)
    dec = _decoder(V, beam, 0.99, 40)
    n = min(10, beam)
    off = dec._batch([probs], want_tokens=True, nbest=min(n + 1, beam))[0]
    dec.reset_decoder()
    for lo in range(0, T, 16):
        k = min(16, T - lo)
        out = dec.decode_chunk(probs[None, lo:lo + k], np.array([k]), nbest=n)
        toks, lens, scores = (t.cpu().numpy() for t in dec._gout)                     # what masr_gbeam_advance itself wrote
        assert dec.last_nbest_tokens[0] == toks[0, :lens[0]].tolist() == dec.last_tokens
        assert np.float32(dec.last_nbest[0][0]).view(np.uint32) == scores.view(np.uint32)[0] and out == dec.last_nbest[0]
        assert 1 <= len(dec.last_nbest) <= n
    stream = [(t, s) for t, (s, _) in zip(dec.last_nbest_tokens, dec.last_nbest)]
    compare(stream, off, n)
    # a reset stream has no live set until its next advance
    dec.reset_decoder()
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert _lib.lib().masr_gbeam_nbest(dec._geng.h, dec._gstream, 1, p, 8, p, p, p, None) != 0
    msg = _lib.lib().masr_last_error().decode()
    assert 'masr_gbeam_nbest' in msg and 'no masr_gbeam_advance' in msg, msg


@pytest.mark.gpu
def test_refusals_by_name(tmp_path):
    import torch
    from masr_amd import _lib, runtime
    lib = _lib.lib()
    eng = runtime.aux_engine()
    name, probs, beam, cut, topn = all_cases()[1]
    dec = _decoder(probs[0].shape[1], beam, cut, topn)
    one, rows, count, max_len = gpu_search_and_nbest(dec, probs, 3)
    B = len(probs)
    out = torch.full((B * (beam + 1) * (max_len + 3),), -7, dtype=torch.int32, device=eng.device)
    p = C.c_void_p(out.data_ptr())
    here = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lm_dec, _, _ = _lm_decoder(tmp_path, probs[0].shape[1], beam, cut, topn, order=3)

    def refused(match, B_=B, beam_=beam, n=3, lm=None, max_len_=max_len, stream=here):
        rc = lib.masr_beam_nbest_gpu(eng.h, B_, beam_, n, lm, C.c_float(0.0), C.c_float(0.0), p, max_len_, p, p, p, stream)
        assert rc != 0
        msg = lib.masr_last_error().decode()
        assert 'masr_beam_nbest_gpu' in msg and match in msg, msg

    refused('B = 3', B_=B + 1)
    refused(f'beam_size = {beam - 1}', beam_=beam - 1)
    refused('language model', lm=lm_dec._ext_scorer.h)
    refused('nbest = 0', n=0)
    refused(f'nbest = {beam + 1}', n=beam + 1)
    refused('max_len', max_len_=0)
    other = torch.cuda.Stream()
    refused('no masr_beam_search_gpu has run on this stream', stream=C.c_void_p(other.cuda_stream))
    torch.cuda.synchronize()
    assert bool((out == -7).all())                     # nothing was launched
    # a search with the scorer bound, then a call without it
    gpu_search_and_nbest(lm_dec, probs, 3)
    refused('had a language model bound')
    # ... and with it, but not with the weights that search ran with (2.2 / 4.3): entry 0 would not be its score
    rc = lib.masr_beam_nbest_gpu(eng.h, B, beam, 3, lm_dec._ext_scorer.h, C.c_float(1.0), C.c_float(4.3), p, max_len, p, p, p, here)
    assert rc != 0 and 'are not the weights of the last search' in lib.masr_last_error().decode()
