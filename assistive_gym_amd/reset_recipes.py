"""What <Task>Env.reset is made of, per task kind: one row that the pool builder (vec_env.build_reset_pool), the batched environment's in-place
reset (AssistiveVecEnv._fresh_reset) and the scalar environments (envs.AssistiveEnv.reset) all read.  A new task is one row here and one
sampler body under host/."""
import importlib
from collections import namedtuple

from .blob import ModelBlob
from .libagx import Stepper
from .model import compiler as L

RAGDOLL_SETTLE_STEPS = 100   # bed_bathing.py:130-131
ARM_FALL_STEPS = 100         # arm_manipulation.py:145-146
ARM_DROP_BASE = (-0.25, 0.2, 0.95)   # arm_manipulation.py:123

# settle_steps: the simulation steps reset() runs after the sampling, on the task's own model
# aux:          the settles BEFORE the sampling, on further models attached to the stepper (attach_settle_models)
# no_tremor:    impairment 'random' means 'no_tremor' (build_assistive_env(human_impairment='no_tremor'), arm_manipulation.py:112)
# extra:        a garment / the water travels with the state record: pools are (states, extra) pairs
# fused:        the device entry point of a POOL: agx_reset (sampling + settle in one call) or agx_sample_reset, then agx_settle
# redraw:       pool entries that come out of the settle non-finite are drawn again (build_reset_pool)
# host:         the numpy sampler's module under host/, and the device helpers its make_states takes (HELPERS)
# host_settle:  the settle_steps of a host-sampled state run on the stepper it is injected into (dressing: inside make_states, by its ClothSettler)
Recipe = namedtuple('Recipe', 'settle_steps aux no_tremor extra fused redraw host helpers host_settle')
RECIPES = {
    L.TASK_FEEDING: Recipe(25, None, False, False, False, True, 'reset', ('checker',), True),                                  # feeding.py:178-179
    L.TASK_DRINKING: Recipe(50, None, False, True, True, False, 'reset_drinking', (), True),                                   # drinking.py:176-177: the water drops into the cup
    L.TASK_DRESSING: Recipe(50, None, False, True, True, False, 'reset_dressing', ('cloth', 'checker'), False),                # dressing.py:186-187
    L.TASK_SCRATCH_ITCH: Recipe(0, None, False, False, False, False, 'reset_scratch', ('checker',), False),                    # ScratchItchEnv.reset has no settle loop
    L.TASK_BED_BATHING: Recipe(0, 'ragdoll', False, False, False, False, 'reset_bed', ('ragdoll', 'checker'), False),          # bed_bathing.py:119-137
    L.TASK_ARM_MANIPULATION: Recipe(0, 'arm_fall', True, False, False, False, 'reset_arm', ('ragdoll', 'arm_fall', 'checker'), False),   # arm_manipulation.py:117-146
}
SETTLE_STEPS = RECIPES[L.TASK_FEEDING].settle_steps


def recipe(blob):
    return RECIPES[blob.task_kind]


def impairment_of(blob, impairment):
    return 'no_tremor' if recipe(blob).no_tremor and impairment == 'random' else impairment


# ---- the device side ---------------------------------------------------------------------------------------------------------------------------
def attach_ragdoll_model(stepper, n_envs, device):
    """bed bathing: the stepper's reset generator reads the human's resting pose from the settled records of a second model, the rag doll
    (bed_bathing.py:119-137): a Stepper on `bed_settle` with as many environments, attached through agx_attach_settle_model"""
    rag = Stepper(ModelBlob.load('bed_settle'), n_envs, device)
    stepper.attach_settle_model(rag, RAGDOLL_SETTLE_STEPS)
    return rag


def attach_arm_fall_models(stepper, blob, n_envs, device):
    """arm manipulation: ArmManipulationEnv.reset has TWO settles (arm_manipulation.py:117-146) -- the rag doll (bed_settle,
    dropped from its own spot) and the fall of the posed right arm, which runs on the task's own model at the reset's gravity of -1
    (ModelBlob.fall_model()).  The fall handle is attached to the task's, the rag doll to the fall handle.  -> (fall, ragdoll) steppers"""
    rag = Stepper(ModelBlob.load('bed_settle').with_drop_base(ARM_DROP_BASE), n_envs, device)
    fall = Stepper(blob.fall_model(), n_envs, device)
    fall.attach_settle_model(rag, RAGDOLL_SETTLE_STEPS)
    stepper.attach_settle_model(fall, ARM_FALL_STEPS)
    return fall, rag


def attach_settle_models(stepper, blob, n_envs, device):
    """the row's `aux` models, where the blob's reset section asks for them (AGX_X_FLAGS 16: a rag doll; 128: the arm's fall with the rag doll
    behind it) -> the further steppers, which the caller closes"""
    if not blob.has_reset_generator:
        return ()
    flags = int(blob.i[int(blob.i[L.H['OFF_RESET']]) + L.X_['FLAGS']])
    if recipe(blob).aux == 'arm_fall' and flags & 128:
        return attach_arm_fall_models(stepper, blob, n_envs, device)
    return (attach_ragdoll_model(stepper, n_envs, device),) if flags & 16 else ()


def sample_on_device(stepper, blob, seed, impairment, fused):
    """the whole of reset() on the device, every environment of the stepper from seed + its index"""
    steps = recipe(blob).settle_steps
    if fused:
        stepper.reset(None, None, seed, impairment=impairment, settle_substeps=steps)
    else:
        stepper.sample_reset(seed, impairment=impairment)
        if steps > 0:
            stepper.settle(steps)


# ---- the host side -----------------------------------------------------------------------------------------------------------------------------
def _helper(name, blob, n, device):
    from .host.reset_arm import ArmFallSettler
    from .host.reset_bed import DeviceCollisionChecker, RagdollSettler
    from .host.reset_dressing import ClothSettler
    if name == 'checker':                 # init_robot_pose's collision rejection: only a robot that is placed can be placed again (host/reset.py)
        placed = blob.task_kind != L.TASK_FEEDING or blob.meta.get('mount') in ('toc', 'mobile')
        return 'checker', DeviceCollisionChecker(blob, n, device) if placed else None
    return {'ragdoll': lambda: ('settler', RagdollSettler(n, device)), 'arm_fall': lambda: ('arm_settler', ArmFallSettler(blob, n, device)),
            'cloth': lambda: ('settler', ClothSettler(blob, n, device))}[name]()


class HostSampler:
    """The task's numpy sampler (host/<row.host>.make_states) with the device helpers its row names, built once for batches of up to n."""

    def __init__(self, blob, n, device=0):
        self.blob, self.row = blob, recipe(blob)
        self.make_states = importlib.import_module('.host.' + self.row.host, __package__).make_states
        self.helpers = dict(_helper(name, blob, n, device) for name in self.row.helpers)

    def __call__(self, n, seed, impairment='random'):
        """-> (states, garments / water or None), to be injected into a stepper (inject)"""
        out = self.make_states(self.blob, n, seed=seed, impairment=impairment_of(self.blob, impairment), **self.helpers)
        return (out[0], out[1]) if self.row.extra else (out[0], None)

    def inject(self, stepper, states, extra):
        """host-sampled states into a stepper of as many environments, and the row's settle where the sampler has not run it"""
        stepper.set_state(states)
        if extra is not None:
            stepper.set_cloth(extra)
        if self.row.host_settle and self.row.settle_steps > 0:
            stepper.settle(self.row.settle_steps)
