"""python evaluate.py --task=T1 --checkpoint=PATH [--num_envs N] [--seed S] [--steps K] [--out FILE] [--gait] [--record_out FILE.npz]

How well a checkpoint walks (README "Evaluation"): the policy's mean action drives every robot through its first episode under envs/<task>.yaml as
it stands, one HIP launch per env step keeps a per-robot record, and the report -- falls, time-outs, tracking RMSE per command class, distance,
joint power, for all robots and per terrain level / column -- is printed as a table and written as JSON.  Any checkpoint of this build: Runner's
(frame stack, perceptive actor, observation normaliser) under the config it was trained with, a distilled student's under its teacher's.  One GPU.
--gait keeps a second per-robot record (one more launch per step) and prints a second table: action rate, effort, body wobble, duty factor, step
frequency, left/right asymmetry, foot slip, touchdown force, swing clearance, cost of transport.  --record_out saves the per-robot records."""
from booster_gym_amd.utils.evaluate import main

if __name__ == "__main__":
    main()
