"""-m gpu: the launch layer of libagx (csrc/agx_api.hip).  agx_step_timed issues the work of agx_step -- the same chunks, the same kernels, the
same arguments -- so the two end in the same bits at every chunk count; the chunk count that the library reports is the one that it launches;
and a reset of a subset of the environments through attached handles (rag doll, arm fall) leaves every other environment of every handle alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    from assistive_gym_amd import libagx
    if libagx.load().agx_device_count() <= 0:
        __import__('conftest').no_gpu()
    return libagx


# (environments, AGX_CHUNKS, chunks that result): one chunk below 64 environments per chunk, an even split, the ragged tail (67 + 67 + 66),
# the clamp to 8, and the default of three chunks from 2048 environments on
CHUNK_CASES = [(64, None, 1), (127, '2', 1), (130, '2', 2), (192, '3', 3), (200, '3', 3), (640, '9', 8), (2048, None, 3)]


@pytest.mark.parametrize('n,chunks,nc', CHUNK_CASES, ids=['%d-%s' % (n, c or 'default') for n, c, _ in CHUNK_CASES])
def test_timed_step_is_the_step(gpu, blob, monkeypatch, n, chunks, nc):
    import torch
    if chunks is None:
        monkeypatch.delenv('AGX_CHUNKS', raising=False)
    else:
        monkeypatch.setenv('AGX_CHUNKS', chunks)       # read in agx_create
    A, B = gpu.Stepper(blob, n), gpu.Stepper(blob, n)
    A.sample_reset(4321); A.settle(25); A.synchronize()
    B.set_state(A.get_state())
    assert A.n_chunks() == nc and B.n_chunks() == nc
    frame_skip = int(blob.param('FRAME_SKIP'))
    rng = np.random.RandomState(7)
    outs = [[torch.zeros((n, blob.obs_dim), device='cuda'), torch.zeros(n, device='cuda'), torch.zeros(n, dtype=torch.uint8, device='cuda'),
             torch.zeros((n, 8), device='cuda')] for _ in range(2)]
    for k in range(3):
        act = torch.as_tensor(rng.uniform(-1, 1, (n, blob.act_dim)).astype(np.float32), device='cuda')
        A.step_dev(act, *outs[0]); A.synchronize()
        ms, cnt = B.step_timed(act, *outs[1])
        assert cnt == [nc * frame_skip, nc * frame_skip, nc], (k, cnt)
        assert all(np.isfinite(t) and t > 0 for t in ms), (k, ms)
        for a, b, what in zip(outs[0], outs[1], ('obs', 'reward', 'done', 'info')):
            np.testing.assert_array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8), err_msg='%s, step %d' % (what, k))
        np.testing.assert_array_equal(A.get_state().view(np.uint32), B.get_state().view(np.uint32), err_msg='states, step %d' % k)
    A.close(); B.close()


def test_timed_step_runs_every_internal_substep(gpu, blob, monkeypatch):
    """A model whose p.stepSimulation() is more than one internal substep long (AGX_H_SIM_SUBSTEPS; the committed ones all carry a cloth or water
    section, which agx_step_timed refuses): FeedingJaco with two internal substeps and a frame skip of two.  The timed step issues the
    frame_skip x SIM_SUBSTEPS [build, solve] pairs of agx_step per chunk and ends in its bits."""
    import torch
    from assistive_gym_amd.blob import ModelBlob
    from assistive_gym_amd.model import compiler as L
    monkeypatch.setenv('AGX_CHUNKS', '2')
    w = blob.set_param('FRAME_SKIP', 2.0).words.copy()
    w.view(np.int32)[L.H['SIM_SUBSTEPS']] = 2
    b = ModelBlob(w, blob.meta)
    n = 130
    ref = gpu.Stepper(blob, n)
    ref.sample_reset(99); ref.settle(25); ref.synchronize()
    A, B = gpu.Stepper(b, n), gpu.Stepper(b, n)
    A.set_state(ref.get_state()); B.set_state(ref.get_state())
    rng = np.random.RandomState(3)
    outs = [[torch.zeros((n, b.obs_dim), device='cuda'), torch.zeros(n, device='cuda'), torch.zeros(n, dtype=torch.uint8, device='cuda'),
             torch.zeros((n, 8), device='cuda')] for _ in range(2)]
    for k in range(2):
        act = torch.as_tensor(rng.uniform(-1, 1, (n, b.act_dim)).astype(np.float32), device='cuda')
        A.step_dev(act, *outs[0]); A.synchronize()
        ms, cnt = B.step_timed(act, *outs[1])
        assert cnt == [2 * 4, 2 * 4, 2], cnt
        for x, y in zip(outs[0], outs[1]):
            np.testing.assert_array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
        np.testing.assert_array_equal(A.get_state().view(np.uint32), B.get_state().view(np.uint32))
    for s in (ref, A, B):
        s.close()


@pytest.mark.parametrize('n', [64, 2048])
def test_particle_models_run_in_one_chunk_and_are_not_timed(gpu, monkeypatch, n):
    import torch
    from assistive_gym_amd.blob import ModelBlob
    monkeypatch.delenv('AGX_CHUNKS', raising=False)
    b = ModelBlob.load('drinking_jaco')
    st = gpu.Stepper(b, n)
    assert st.n_chunks() == 1
    if n == 64:
        with pytest.raises(gpu.AgxError):
            st.step_timed(torch.zeros((n, b.act_dim), device='cuda'), torch.zeros((n, b.obs_dim), device='cuda'), torch.zeros(n, device='cuda'),
                          torch.zeros(n, dtype=torch.uint8, device='cuda'))
    st.close()


def _chain(gpu, model, n):
    from assistive_gym_amd.blob import ModelBlob
    from assistive_gym_amd.vec_env import attach_arm_fall_models, attach_ragdoll_model
    b = ModelBlob.load(model)
    st = gpu.Stepper(b, n)
    return [st] + ([attach_ragdoll_model(st, n, 0)] if model.startswith('bed_bathing') else list(attach_arm_fall_models(st, b, n, 0)))


@pytest.mark.parametrize('model,n,picked', [('bed_bathing_sawyer', 6, (1, 4)), ('arm_manipulation_sawyer', 4, (0, 2))])
def test_masked_reset_through_attached_handles(gpu, model, n, picked):
    """agx_reset(mask, seeds) on a handle whose reset runs through a rag-doll handle (bed bathing) or a fall handle and a rag-doll handle (arm
    manipulation): on every handle of the chain the environments outside the mask keep their records bit for bit, and those inside end where a
    fresh chain ends that resets every environment from the same seeds"""
    import torch
    chain = _chain(gpu, model, n)
    st = chain[0]
    seeds_a = torch.arange(n, dtype=torch.int64, device='cuda') * 13 + 555000111
    seeds_b = torch.arange(n, dtype=torch.int64, device='cuda') * 7 + 123456789
    st.reset(None, seeds_a)
    for k in range(2):
        st.step_host(np.zeros((n, st.act_dim), dtype=np.float32))
    st.synchronize()
    before = [s.get_state() for s in chain]
    mask = torch.zeros(n, dtype=torch.uint8, device='cuda'); mask[list(picked)] = 1
    m = mask.cpu().numpy().astype(bool)
    st.reset(mask, seeds_b)
    st.synchronize()
    after = [s.get_state() for s in chain]
    fresh = _chain(gpu, model, n)
    fresh[0].reset(None, seeds_b)
    fresh[0].synchronize()
    want = [s.get_state() for s in fresh]
    for k in range(len(chain)):
        np.testing.assert_array_equal(after[k][~m].view(np.uint32), before[k][~m].view(np.uint32), err_msg='handle %d of the chain, outside the mask' % k)
        np.testing.assert_array_equal(after[k][m].view(np.uint32), want[k][m].view(np.uint32), err_msg='handle %d of the chain, inside the mask' % k)
        assert not np.array_equal(after[k][m], before[k][m])          # the masked environments did move
    for s in chain + fresh:
        s.close()
