"""python distill.py --task=T1 --teacher=PATH [--student_frame_stack Hs --max_iterations N --num_envs N --seed S --sim_device cuda:0 --rl_device cuda:0]

Teacher-student distillation (README "Distillation"): the perceptive actor of checkpoint PATH (trained with terrain.actor_heights) is distilled into an
actor that sees the 47 x env.frame_stack observation columns only.  The config is the teacher's (envs/<task>.yaml with terrain.actor_heights: true);
its `distillation:` section holds the rest, --teacher overrides distillation.teacher_checkpoint and --student_frame_stack
distillation.student_frame_stack (a student that sees the env's last Hs observations, more than its teacher's env.frame_stack).  One GPU."""
from booster_gym_amd.utils.distill import Distiller

if __name__ == "__main__":
    Distiller().train()
