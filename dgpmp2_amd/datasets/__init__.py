from .planning_dataset import PlanningDataset, write_environment, write_problem, write_meta
from .problem_generation import sample_problems, generate_dataset
