from .planning_dataset import PlanningDataset, write_environment, write_problem, write_meta
from .problem_generation import sample_problems, generate_dataset, init_paths, shortcut_paths, prior_samples, lift_headings, PathInfo, ShortcutInfo, PriorSampleInfo, HeadingInfo
from .obstacle_maps import generate_obstacle_maps, dataset_params, reference_separations, confs_to_pixels, ObstacleInfo
